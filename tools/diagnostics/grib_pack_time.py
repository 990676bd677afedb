"""Times the device side of the native GRIB output -- ops.grib_pack, every packed feature of every lead time of all B samples, and
the pinned copy of params + bit streams -- against the device-side sequence of the reference's predict_step /
save_named_tensors_to_grib (py4cast/lightning.py:1164-1169, io/outputs.py:146-193) restated with library operations on the same GPU
in the same process: per feature the in-place ``*= std`` and ``+= mean`` on the strided feature column of the whole prediction, then
per sample, lead time and written feature the strided plane gather ``[:, :, idx]`` with a blocking .cpu().  The reference's host side
(eccodes finds the range and packs, through epygram) cannot be timed here: neither library is installed; it is OUTSIDE the comparison.

    python tools/diagnostics/grib_pack_time.py [--out profiles/grib_pack.txt]

Both sides: host clock around one call ending in a synchronise (the reference's sequence ends in blocking copies anyway), 3
alternating rounds of 10 native / 3 reference calls after warm-up calls, median of the rounds' medians.  The native call also with
device events (median of 7 windows of 20 calls).  The three launches of the call are told apart by a kernel trace of this script
(``rocprofv3 --kernel-trace --stats -- python tools/diagnostics/grib_pack_time.py --trace-only``: a run of its own, the averages go
into the file by hand); the bytes of each pass -- prediction read once per pass (whole points in the dense form; in the gather form a 64-byte line per
packed feature and point, at most the whole point: the same count ops.grib_pack states), stream bytes written by the pack pass -- are
printed here so that the rates follow from the trace."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from py4cast_amd import _lib as L  # noqa: E402
from py4cast_amd import ops  # noqa: E402

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


def reference_sequence(pred, std, mean, features):
    """lightning.py:1164-1169 on the whole batch, then io/outputs.py:189-193 per sample, lead time and written feature.  std < 1 keeps
    the repeated in-place rescale of the same buffer bounded."""
    F = pred.shape[-1]
    for idx in range(F):
        pred[:, :, :, :, idx] *= std[idx]
        pred[:, :, :, :, idx] += mean[idx]
    out = []
    for sample in pred:
        for step in sample:
            for idx in features:
                out.append(step[:, :, idx].cpu().numpy())
    return out


def shape_report(title, B, T, H, W, F, features, lines, rounds=3, trace_only=False):
    K, N = len(features), H * W
    g = torch.Generator(device=dev).manual_seed(0)
    pred = torch.randn(B, T, H, W, F, device=dev, generator=g)
    work = pred.clone()
    std, mean = torch.rand(F, device=dev, generator=g) * 0.5 + 0.5, torch.randn(F, device=dev, generator=g)
    spec = [(2, 16)] * K                                                  # the usual template: 16 bits, two decimals
    pitch = ops.grib_pitch(N, spec)
    pbytes = B * T * K * ops.GRIB_PARAMS * 4
    buf = torch.empty(pbytes + B * T * K * pitch, dtype=torch.uint8, device=dev)
    out = (buf[:pbytes].view(torch.int32).view(B, T, K, ops.GRIB_PARAMS), buf[pbytes:].view(B, T, K, pitch))

    def native():
        return ops.grib_pack(pred, std, mean, spec, features=features, out=out)

    if trace_only:
        for _ in range(25):
            native()
        torch.cuda.synchronize()
        return

    def reference():
        return reference_sequence(work, std, mean, features)

    wall_us(native, n=3), wall_us(reference, n=1)
    nat, ref = [], []
    for _ in range(rounds):
        nat.append(wall_us(native, n=10))
        ref.append(wall_us(reference, n=3))
    n_us, r_us = statistics.median(nat), statistics.median(ref)
    d_us = device_us(native)
    host = torch.empty(buf.numel(), dtype=torch.uint8, pin_memory=True)
    c_us = wall_us(lambda: host.copy_(buf, non_blocking=True), n=10, warm=3)
    planes = torch.empty(B * T * K * N, dtype=torch.float32, device=dev)
    host32 = torch.empty(planes.numel(), dtype=torch.float32, pin_memory=True)
    p_us = wall_us(lambda: host32.copy_(planes, non_blocking=True), n=10, warm=3)
    dense = bool(L.lib().p4c_grib_pack_dense(K, F))
    read = B * T * N * (4 * F if dense else min(4 * F, 64 * K))
    useful = B * T * N * 4 * K
    stream = B * T * K * ((N * 16 + 7) // 8)
    lines.append(f"{title}: {B}x{T}x{H}x{W}x{F}, {K} features packed ({'dense' if dense else 'gather'} form), 16 bits, D = 2, n = B: "
                 f"prediction {pred.numel() * 4 / 1e6:.1f} MB, streams {stream / 1e6:.1f} MB")
    lines.append(f"  grib_pack, host clock to a synchronise                         {n_us:10.1f} us   (rounds {' '.join(f'{v:.0f}' for v in nat)})")
    lines.append(f"  the reference's device-side sequence, same clock               {r_us:10.1f} us   (rounds {' '.join(f'{v:.0f}' for v in ref)})   "
                 f"ratio {r_us / n_us:.1f}")
    lines.append(f"  device events, the whole call (range + finish + pack)          {d_us:10.1f} us   "
                 f"{(2 * read + stream) / d_us / 1e6:5.2f} TB/s of two prediction reads + streams written")
    lines.append(f"  bytes per pass: range reads {read / 1e6:.1f} MB ({useful / 1e6:.1f} MB of them packed values); pack reads the same and writes "
                 f"{stream / 1e6:.1f} MB")
    lines.append(f"  pinned copy of params + streams ({buf.numel() / 1e6:.1f} MB), to a synchronise {c_us:10.1f} us   {buf.numel() / c_us / 1e3:5.1f} GB/s")
    lines.append(f"  pinned copy of the same fields as fp32 planes ({planes.numel() * 4 / 1e6:.1f} MB)        {p_us:10.1f} us   "
                 f"{planes.numel() * 4 / p_us / 1e3:5.1f} GB/s   (what OutputStager ships)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "grib_pack.txt"))
    ap.add_argument("--trace-only", action="store_true", help="only 25 native calls per shape, for a kernel trace")
    args = ap.parse_args()
    lines = [f"GRIB2 simple packing on the device: tools/diagnostics/grib_pack_time.py on {torch.cuda.get_device_name(0)}",
             "call and reference: host clock around one call ending in a synchronise, 3 alternating rounds of 10 / 3 calls, median of the "
             "rounds' medians; the whole call also with device events, median of 7 windows of 20 calls", ""]
    shape_report("benchmark shape", 2, 3, 512, 512, 60, tuple(range(60)), lines, trace_only=args.trace_only)
    lines.append("")
    # Titan's 21 features, of which the reference writes six: t2m, u10, v10, prmsl, r2, tp
    shape_report("Titan shape", 2, 3, 512, 640, 21, (0, 3, 4, 9, 12, 17), lines, trace_only=args.trace_only)
    if args.trace_only:
        return
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
