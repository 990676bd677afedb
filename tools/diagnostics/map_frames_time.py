"""Times the device side of the native prediction-map observers -- ops.map_planes + ops.map_render, n = 1 sample, K = 4 variables --
against the device-side sequence of the reference's MapPlot.update / plot_prediction (py4cast/plots.py:260-328, 113-163) restated
with library operations in the same process: the copies of prediction, target and batch, pred * mask, the two rescales, the
min / max over the flattened target and the 2 T K strided (H,W) planes fetched with a blocking .cpu().

    python tools/diagnostics/map_frames_time.py [--out profiles/map_frames.txt]

Both sides: host clock around one call ending in a synchronise (the reference's sequence ends in blocking copies anyway), 5
alternating rounds of 20 calls after 5 warm-up calls each, median of the rounds' medians.  The native pair also with device events
(median of 7 windows of 50 calls).  The pinned copy of frames + ranges and the observer's whole device side (planes, render, copy,
wait) are timed on their own.  The host figure work (matplotlib, savefig) is OUTSIDE the comparison -- both sides do it -- and is
reported separately."""
import argparse
import os
import statistics
import sys
import tempfile
import time
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from py4cast_amd import _lib as L  # noqa: E402
from py4cast_amd import observers, ops  # noqa: E402
from py4cast_amd.namedtensor import NamedTensor  # noqa: E402

dev = torch.device("cuda:0")


def wall_us(fn, n=20, warm=0):
    out = []
    for i in range(warm + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def device_us(fn, n=50, windows=7, warm=10):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / n * 1000)
    return statistics.median(out)


def reference_sequence(pred, target, mask, batch, std, mean, n, K):
    """plots.py:271-273, 299-300, 311-312 and the .cpu() of plot_prediction per (lead time, variable, panel)"""
    p = pred.clone() * mask
    t = target.clone()
    _ = [b.clone() for b in batch]
    pr, tr = p * std + mean, t * std + mean
    out = []
    for ps, ts in zip(pr[:n], tr[:n]):
        out.append(ts.flatten(0, 2).min(dim=0)[0].cpu())
        out.append(ts.flatten(0, 2).max(dim=0)[0].cpu())
        for pt, tt in zip(ps, ts):
            for k in range(K):
                out.append(pt[:, :, k].cpu())
                out.append(tt[:, :, k].cpu())
    return out


class Stats:
    def __init__(self, std, mean):
        self.d = {"std": std.cpu(), "mean": mean.cpu()}

    def to_list(self, stat, names, dtype=torch.float32):
        return self.d[stat].type(dtype)


def shape_report(title, B, T, H, W, F, lines, n=1, K=4, rounds=5):
    g = torch.Generator(device=dev).manual_seed(0)
    pred = torch.randn(B, T, H, W, F, device=dev, generator=g)
    target = torch.randn(B, T, H, W, F, device=dev, generator=g)
    mask = torch.ones_like(target)
    batch = [torch.randn(B, 1, H, W, F, device=dev, generator=g), torch.randn(B, T, H, W, 5, device=dev, generator=g), target]
    std, mean = torch.rand(F, device=dev, generator=g) + 0.5, torch.randn(F, device=dev, generator=g)
    interior = torch.ones(H, W, device=dev)
    interior[:8] = interior[-8:] = 0
    lut = torch.from_numpy(observers.plasma_table() if observers.plasma_table() is not None else
                           torch.arange(768, dtype=torch.uint8).reshape(256, 3).numpy()).to(dev)
    none, f32 = ops.MaskSpec(L.MASK_NONE), ops.MaskSpec(L.MASK_F32, mask)

    def native(spec=none):
        planes, vrange = ops.map_planes(pred, target, spec, std, mean, range(K), n)
        return ops.map_render(planes, vrange, lut, interior.reshape(-1), H, W), vrange

    def reference():
        return reference_sequence(pred, target, mask, batch, std, mean, n, K)

    wall_us(native, n=5), wall_us(reference, n=5)
    nat, ref = [], []
    for _ in range(rounds):
        nat.append(wall_us(native))
        ref.append(wall_us(reference))
    n_us, r_us = statistics.median(nat), statistics.median(ref)
    planes, vrange = ops.map_planes(pred, target, none, std, mean, range(K), n)
    p_us = device_us(lambda: ops.map_planes(pred, target, none, std, mean, range(K), n))
    pm_us = device_us(lambda: ops.map_planes(pred, target, f32, std, mean, range(K), n))
    d_us = device_us(lambda: ops.map_render(planes, vrange, lut, interior.reshape(-1), H, W))
    frames, _ = native()
    host = torch.empty(frames.numel() + 4 * vrange.numel(), dtype=torch.uint8, pin_memory=True)
    packed = torch.empty(host.shape, dtype=torch.uint8, device=dev)
    c_us = wall_us(lambda: host.copy_(packed, non_blocking=True), n=30, warm=5)
    names = [f"v{i}" for i in range(F)]
    obj = types.SimpleNamespace(stats=Stats(std, mean), interior_2d=interior[:, :, None], trainer=types.SimpleNamespace(is_global_zero=True))
    dims = ["batch", "timestep", "lat", "lon", "features"]
    plotter = observers.PredictionTimestepPlot(n, K, lut=lut.cpu().numpy())
    pn, tn = NamedTensor(pred, dims, names), NamedTensor(target, dims, names)
    o_us = wall_us(lambda: plotter.render(obj, pn, tn, None, n, K), n=30, warm=5)
    plane_bytes, frame_bytes = 4 * n * T * K * 2 * H * W, frames.numel()
    lines.append(f"{title}: {B}x{T}x{H}x{W}x{F}, n = {n}, K = {K}: planes {plane_bytes / 1e6:.1f} MB, frames {frame_bytes / 1e6:.1f} MB")
    lines.append(f"  map_planes + map_render, host clock to a synchronise   {n_us:9.1f} us   (rounds {' '.join(f'{v:.0f}' for v in nat)})")
    lines.append(f"  the reference's device-side sequence, same clock       {r_us:9.1f} us   (rounds {' '.join(f'{v:.0f}' for v in ref)})   ratio {r_us / n_us:.1f}")
    lines.append(f"  p4c_map_planes, device events                          {p_us:9.1f} us   (explicit fp32 mask: {pm_us:.1f} us)")
    lines.append(f"  p4c_map_render, device events                          {d_us:9.1f} us   {(plane_bytes + frame_bytes) / d_us / 1e6:5.2f} TB/s of planes read + frames written")
    lines.append(f"  pinned copy of frames + ranges ({host.numel() / 1e6:.1f} MB), to a synchronise {c_us:7.1f} us   {host.numel() / c_us / 1e3:5.1f} GB/s")
    lines.append(f"  MapPlot.render: planes, render, copy, wait             {o_us:9.1f} us")
    return frames, vrange


def figure_report(frames, vrange, lines):
    if observers._pyplot() is None:
        lines.append("host figure work: matplotlib absent, not measured")
        return
    frame, lo, hi = frames[0, 0, 0].cpu().numpy(), float(vrange[0, 0, 0]), float(vrange[0, 0, 1])
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(6):
            t0 = time.perf_counter()
            fig = observers.plot_prediction_frame(frame, lo, hi, title="t2m (K), t=1 (3 h)")
            fig.savefig(os.path.join(tmp, f"{i}.png"))
            out.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"host figure work, outside the comparison: one {frame.shape[0]}x{frame.shape[1]} frame -> matplotlib figure + savefig "
                 f"{statistics.median(out[1:]):.0f} ms (median of 5; a step makes T x K of them)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "map_frames.txt"))
    args = ap.parse_args()
    lines = [f"prediction-map frames on the device: tools/diagnostics/map_frames_time.py on {torch.cuda.get_device_name(0)}",
             "pair and reference: host clock around one call ending in a synchronise, 5 alternating rounds of 20 calls, median of the "
             "rounds' medians; kernels: device events, median of 7 windows of 50 calls", ""]
    shape_report("benchmark shape", 2, 3, 512, 512, 60, lines)
    lines.append("")
    frames, vrange = shape_report("Titan shape", 2, 3, 512, 640, 21, lines)
    lines.append("")
    figure_report(frames, vrange, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
