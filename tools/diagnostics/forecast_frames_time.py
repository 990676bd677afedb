"""Times the device side of the native forecast GIFs -- ops.forecast_frames, every feature of every lead time of all B samples --
against the device-side sequence of the reference's predict_step / save_gifs (py4cast/lightning.py:1164-1169, io/outputs.py:223-227)
restated with library operations on the same GPU in the same process: per feature the in-place ``*= std`` and ``+= mean`` on the
strided feature column of the whole prediction, then per sample and feature the strided gather ``[..., idx]`` with a blocking .cpu().

    python tools/diagnostics/forecast_frames_time.py [--out profiles/forecast_frames.txt]

Both sides: host clock around one call ending in a synchronise (the reference's sequence ends in blocking copies anyway), 3
alternating rounds of 10 native / 3 reference calls after warm-up calls, median of the rounds' medians.  The native call also with
device events (median of 7 windows of 20 calls) in three settings: every feature auto-scaled (range launch, finish launch, index
launch), every range given (the index launch alone), and the shipped display table of the shape's feature names; the range pass is
the difference of the first two.  Bandwidth: prediction bytes read per pass plus frame bytes written, over the event time.  The
pinned copy of frames + ranges is timed on its own.  The host work (PIL's GIF encoder here, one matplotlib figure per frame in the
reference) is OUTSIDE the comparison and reported separately for one GIF."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from py4cast_amd import ops  # noqa: E402
from py4cast_amd.outputs import display_for, palette_for, save_palette_gif  # noqa: E402

dev = torch.device("cuda:0")


def wall_us(fn, n=10, warm=0):
    out = []
    for i in range(warm + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def device_us(fn, n=20, windows=7, warm=5):
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


def reference_sequence(pred, std, mean):
    """lightning.py:1164-1169 on the whole batch, then io/outputs.py:226 per sample and feature.  std < 1 keeps the repeated in-place
    rescale of the same buffer bounded."""
    F = pred.shape[-1]
    for idx in range(F):
        pred[:, :, :, :, idx] *= std[idx]
        pred[:, :, :, :, idx] += mean[idx]
    out = []
    for sample in pred:
        for idx in range(F):
            out.append(sample[:, :, :, idx].cpu())
    return out


def shape_report(title, B, T, H, W, names, lines, rounds=3):
    F = len(names)
    g = torch.Generator(device=dev).manual_seed(0)
    pred = torch.randn(B, T, H, W, F, device=dev, generator=g)
    work = pred.clone()
    std, mean = torch.rand(F, device=dev, generator=g) * 0.5 + 0.5, torch.randn(F, device=dev, generator=g)
    auto = [(None, None, None, None)] * F
    given = [(None, None, -3.0, 3.0)] * F
    table = display_for(names)
    frames = torch.empty(B, T, F, H, W, dtype=torch.uint8, device=dev)
    vrange = torch.empty(B, T, F, 2, device=dev)

    def native(display=table):
        return ops.forecast_frames(pred, std, mean, display, out=(frames, vrange))

    def reference():
        return reference_sequence(work, std, mean)

    wall_us(native, n=3), wall_us(reference, n=1)
    nat, ref = [], []
    for _ in range(rounds):
        nat.append(wall_us(native, n=10))
        ref.append(wall_us(reference, n=3))
    n_us, r_us = statistics.median(nat), statistics.median(ref)
    a_us = device_us(lambda: native(auto))
    g_us = device_us(lambda: native(given))
    t_us = device_us(native)
    pred_bytes, frame_bytes = pred.numel() * 4, frames.numel()
    host = torch.empty(frame_bytes + 4 * vrange.numel(), dtype=torch.uint8, pin_memory=True)
    packed = torch.empty(host.shape, dtype=torch.uint8, device=dev)
    c_us = wall_us(lambda: host.copy_(packed, non_blocking=True), n=10, warm=3)
    n_auto = sum(1 for d in table if d.vmin is None or d.vmax is None)
    lines.append(f"{title}: {B}x{T}x{H}x{W}x{F}, all features, n = B: prediction {pred_bytes / 1e6:.1f} MB, frames {frame_bytes / 1e6:.1f} MB; "
                 f"shipped display table: {n_auto} of {F} features auto-scaled")
    lines.append(f"  forecast_frames (shipped table), host clock to a synchronise   {n_us:10.1f} us   (rounds {' '.join(f'{v:.0f}' for v in nat)})")
    lines.append(f"  the reference's device-side sequence, same clock               {r_us:10.1f} us   (rounds {' '.join(f'{v:.0f}' for v in ref)})   "
                 f"ratio {r_us / n_us:.1f}")
    lines.append(f"  device events, shipped table (range + finish + index)          {t_us:10.1f} us")
    lines.append(f"  device events, every feature auto-scaled                       {a_us:10.1f} us   "
                 f"{(2 * pred_bytes + frame_bytes) / a_us / 1e6:5.2f} TB/s of two prediction reads + frames written")
    lines.append(f"  device events, every range given: the index launch alone       {g_us:10.1f} us   "
                 f"{(pred_bytes + frame_bytes) / g_us / 1e6:5.2f} TB/s of prediction read + frames written")
    lines.append(f"  range + finish launches (difference of the two)                {a_us - g_us:10.1f} us   "
                 f"{pred_bytes / max(a_us - g_us, 1e-3) / 1e6:5.2f} TB/s of prediction read")
    lines.append(f"  pinned copy of frames + ranges ({host.numel() / 1e6:.1f} MB), to a synchronise {c_us:10.1f} us   {host.numel() / c_us / 1e3:5.1f} GB/s")
    return frames, table


def gif_report(frames, table, lines):
    clip = frames[0, :, 0].cpu().numpy()
    palette = palette_for(table[0].cmap)
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(6):
            t0 = time.perf_counter()
            save_palette_gif(os.path.join(tmp, f"{i}.gif"), clip, palette)
            out.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"host work, outside the comparison: one GIF of {clip.shape[0]} frames {clip.shape[1]}x{clip.shape[2]} through PIL "
                 f"{statistics.median(out[1:]):.1f} ms (median of 5; a sample makes F of them; the reference draws T x F matplotlib figures "
                 f"per sample, 89 ms per savefig in profiles/map_frames.txt)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "forecast_frames.txt"))
    args = ap.parse_args()
    lines = [f"forecast frames on the device: tools/diagnostics/forecast_frames_time.py on {torch.cuda.get_device_name(0)}",
             "call and reference: host clock around one call ending in a synchronise, 3 alternating rounds of 10 / 3 calls, median of the "
             "rounds' medians; launches: device events, median of 7 windows of 20 calls", ""]
    params = ["t2m", "r2", "tp", "u10", "v10"]
    names60 = [f"aro_{params[i]}_{i}m" if i < 5 else f"aro_p{i}_{i}hpa" for i in range(60)]
    names60[0] = "aro_t2m_2m"
    shape_report("benchmark shape", 2, 3, 512, 512, names60, lines)
    lines.append("")
    names21 = names60[:21]
    frames, table = shape_report("Titan shape", 2, 3, 512, 640, names21, lines)
    lines.append("")
    gif_report(frames, table, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
