"""Times the complex-packing route of the native GRIB output -- ops.grib_pack_complex (templates 5.2 / 5.3) -- against ops.grib_pack
(5.0) at the same widths, on the same prediction, in the same process; the pinned copies of both routes; ForecastGribWriter from
submit to files written for packing="simple" and "complex"; and the bits per value and file sizes of both.

    python tools/diagnostics/grib_pack_complex_time.py [--out profiles/grib_pack_complex.txt]

The prediction is SYNTHETIC: per feature a smooth wave over the grid (amplitude 1 in normalised units) plus white noise of standard
deviation 0.003, about 33 quanta of the 16-bit quantisation.  Bits per value and file sizes are properties of that field, not of real
forecasts.  Calls: device events, median of 7 windows of 20 calls after 5 warm-up calls.  The A/B of the pack pass -- re-read and
re-quantise the prediction (P4C_GRIB_CPX_STORED=0) against reading differences the group pass stored (=1) -- runs on the diagnostic
library, alternating, and the two must give the same bytes.  The launches are told apart by a kernel trace in a run of its own
(``rocprofv3 --kernel-trace --stats -- python tools/diagnostics/grib_pack_complex_time.py --trace-only``)."""
import argparse
import datetime as dt
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grib2_reference as ref  # noqa: E402
from py4cast_amd import _lib as L  # noqa: E402
from py4cast_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
TITAN_NAMES = {0: "aro_t2m_2m", 3: "aro_u10_10m", 4: "aro_v10_10m", 9: "aro_prmsl_0hpa", 12: "aro_r2_2m", 17: "aro_tp_0m"}


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


def wall_us(fn, n=10, warm=3):
    out = []
    for i in range(warm + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def synthetic(B, T, H, W, F):
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.arange(H, device=dev, dtype=torch.float32)[:, None, None] / 97.0
    x = torch.arange(W, device=dev, dtype=torch.float32)[None, :, None] / 131.0
    phase = torch.arange(F, device=dev, dtype=torch.float32)[None, None, :] * 0.7
    smooth = torch.sin(y + phase) * torch.cos(x - 0.5 * phase)
    pred = smooth[None, None] * (1.0 + 0.05 * torch.arange(B * T, device=dev, dtype=torch.float32).view(B, T, 1, 1, 1))
    return (pred + 0.003 * torch.randn(B, T, H, W, F, device=dev, generator=g)).contiguous()


def shape_report(title, B, T, H, W, F, features, lines, trace_only=False):
    K, N = len(features), H * W
    pred = synthetic(B, T, H, W, F)
    g = torch.Generator(device=dev).manual_seed(1)
    std, mean = torch.rand(F, device=dev, generator=g) * 0.5 + 0.5, torch.randn(F, device=dev, generator=g)
    simple, spec = [(2, 16)] * K, [(2, 16, 2)] * K
    pitch = ops.grib_pitch(N, simple)
    sp_bytes = B * T * K * ops.GRIB_PARAMS * 4
    sbuf = torch.empty(sp_bytes + B * T * K * pitch, dtype=torch.uint8, device=dev)
    sout = (sbuf[:sp_bytes].view(torch.int32).view(B, T, K, ops.GRIB_PARAMS), sbuf[sp_bytes:].view(B, T, K, pitch))
    capacity = ops.grib_complex_capacity(B, T, N, spec)
    cp_bytes = B * T * K * ops.GRIB_COMPLEX_PARAMS * 4
    cbuf = torch.empty(cp_bytes + capacity, dtype=torch.uint8, device=dev)
    cout = (cbuf[:cp_bytes].view(torch.int32).view(B, T, K, ops.GRIB_COMPLEX_PARAMS), cbuf[cp_bytes:])

    def simple_call():
        return ops.grib_pack(pred, std, mean, simple, features=features, out=sout)

    def complex_call():
        return ops.grib_pack_complex(pred, std, mean, spec, features=features, out=cout)

    if trace_only:
        for _ in range(25):
            simple_call()
            complex_call()
        torch.cuda.synchronize()
        return
    s_us, c_us = device_us(simple_call), device_us(complex_call)
    params = cout[0].cpu().numpy().reshape(-1, ops.GRIB_COMPLEX_PARAMS)
    used = int(params[-1, 10]) + int(params[-1, 9])
    bits = 8.0 * params[:, 9].astype(np.int64).sum() / (params.shape[0] * N)
    reference_bytes = cout[1][:used].cpu()
    ab = {}
    with L.use_diagnostic_library():
        for _ in range(2):
            for flag in ("0", "1"):
                os.environ["P4C_GRIB_CPX_STORED"] = flag
                ab.setdefault(flag, []).append(device_us(complex_call, windows=5))
                torch.cuda.synchronize()
                assert torch.equal(cout[1][:used].cpu(), reference_bytes), "the two forms of the pack pass differ"
        os.environ.pop("P4C_GRIB_CPX_STORED")
    host = torch.empty(max(sbuf.numel(), cbuf.numel()), dtype=torch.uint8, pin_memory=True)
    copy_s = wall_us(lambda: host[:sbuf.numel()].copy_(sbuf, non_blocking=True))
    copy_p = wall_us(lambda: host[:cp_bytes].copy_(cbuf[:cp_bytes], non_blocking=True))
    copy_c = wall_us(lambda: host[:used].copy_(cbuf[cp_bytes:cp_bytes + used], non_blocking=True))
    dense = bool(L.lib().p4c_grib_pack_dense(K, F))
    lines.append(f"{title}: {B}x{T}x{H}x{W}x{F}, {K} features packed ({'dense' if dense else 'gather'} form), 16 bits, D = 2, order 2 "
                 f"(template 5.3), n = B: prediction {pred.numel() * 4 / 1e6:.1f} MB")
    lines.append(f"  grib_pack (5.0), device events, the whole call (3 launches)          {s_us:10.1f} us")
    lines.append(f"  grib_pack_complex (5.3), device events, the whole call (7 launches)  {c_us:10.1f} us   ratio {c_us / s_us:.2f}")
    lines.append(f"  the pack pass re-reads and re-quantises (diag library)               {statistics.median(ab['0']):10.1f} us   "
                 f"(rounds {' '.join(f'{v:.0f}' for v in ab['0'])})")
    lines.append(f"  the pack pass reads stored differences  (diag library)               {statistics.median(ab['1']):10.1f} us   "
                 f"(rounds {' '.join(f'{v:.0f}' for v in ab['1'])}); workspace + {B * T * K * N * 4 / 1e6:.1f} MB; same bytes")
    lines.append(f"  bits per value of this synthetic field: 16 in 5.0, {bits:.2f} in 5.3 (payloads {used / 1e6:.1f} MB of a capacity of "
                 f"{capacity / 1e6:.1f} MB; 5.0 streams {B * T * K * pitch / 1e6:.1f} MB)")
    lines.append(f"  pinned copy, 5.0: params + streams ({sbuf.numel() / 1e6:.1f} MB), to a synchronise  {copy_s:10.1f} us")
    lines.append(f"  pinned copies, 5.3: params ({cp_bytes / 1e3:.1f} kB) {copy_p:.1f} us + payloads ({used / 1e6:.1f} MB) {copy_c:.1f} us")
    return pred, std, mean


def writer_report(pred, std, mean, features, lines):
    """ForecastGribWriter on the Titan shape, one batch: submit to files written (drain), per packing"""
    from py4cast_amd import grib2
    from py4cast_amd.namedtensor import NamedTensor
    from py4cast_amd.outputs import ForecastGribWriter, GribSample, OutputSavingSettings

    B, T, H, W, F = pred.shape
    names = [TITAN_NAMES.get(f, f"aro_other_{f}") for f in range(F)]
    fields = {"aro_t2m_2m": 0, "aro_u10_10m": 1, "aro_v10_10m": 2, "aro_r2_2m": 3, "aro_prmsl_0hpa": 4, "aro_tp_0m": 5}
    g = np.random.default_rng(3)
    template = b""
    for i in sorted(fields.values()):
        _, category, number, surface, level, D, nbits, pdt = ref.FIELDS[i]
        s4 = ref.section4(category, number, surface, level, template=pdt, end=dt.datetime(2020, 1, 1, 1))
        values = g.standard_normal(H * W).astype(np.float32)
        template += ref.message(0, ref.section1(dt.datetime(2020, 1, 1, 0)), ref.section3(True, ni=W, nj=H), s4, values, D, nbits)
    _, _, lat, lon, _ = grib2.grid_of(grib2.parse_messages(template)[0])        # the forecast grid is the template's
    samples = []
    for b in range(B):
        start = dt.datetime(2023, 1, 1, 6 * b)
        deltas = [dt.timedelta(hours=i - 1) for i in range(T + 2)]
        sample = types.SimpleNamespace(timestamps=types.SimpleNamespace(datetime=start, timedeltas=deltas), member=b,
                                       output_timestamps=types.SimpleNamespace(datetime=start, timedeltas=deltas[2:]))
        samples.append(GribSample.from_sample(sample, start.strftime("%Y%m%d%H")))
    preds = NamedTensor(pred, ["batch", "timestep", "lat", "lon", "features"], names)
    lines.append(f"ForecastGribWriter, Titan shape, one batch of {B} samples x {T} lead times x 6 messages on a {H} x {W} template grid "
                 f"(no bitmap), from submit to the last file written (host clock, median of 5 after 2 warm-up batches):")
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "gribs"))
        with open(os.path.join(root, "template.grib"), "wb") as f:
            f.write(template)
        settings = OutputSavingSettings(template_grib="../template.grib", dir_grib=os.path.join(root, "gribs"), dir_gif=os.path.join(root, "gifs"),
                                        path_to_runtime="{}", grib_fmt="mb{}_ech_{}.grib", grib_identifiers=("member", "leadtime"))
        for packing in ("simple", "complex"):
            writer = ForecastGribWriter(settings, dev, np.repeat(lat[:, None], W, axis=1), np.repeat(lon[None, :], H, axis=0), packing=packing)
            times = []
            for i in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                writer.submit(preds, std, mean, samples)
                writer.drain()
                times.append((time.perf_counter() - t0) * 1e3)
            size = sum(os.path.getsize(p) for p in writer.written[-B * T:])
            lines.append(f"  packing={packing!r:10s} {statistics.median(times[2:]):8.2f} ms   {size / 1e6:6.2f} MB in {B * T} files")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "grib_pack_complex.txt"))
    ap.add_argument("--trace-only", action="store_true", help="only 25 calls of each route per shape, for a kernel trace")
    args = ap.parse_args()
    lines = [f"GRIB2 complex packing on the device: tools/diagnostics/grib_pack_complex_time.py on {torch.cuda.get_device_name(0)}",
             "calls: device events, median of 7 windows of 20 calls after 5 warm-up calls (the A/B of the pack pass: 5 windows, two "
             "alternating rounds).  The prediction is synthetic: a smooth wave of amplitude 1 plus white noise of 0.003 per feature; bits "
             "per value and sizes are properties of that field, not of real forecasts.", ""]
    shape_report("benchmark shape", 2, 3, 512, 512, 60, tuple(range(60)), lines, trace_only=args.trace_only)
    lines.append("")
    titan = shape_report("Titan shape", 2, 3, 512, 640, 21, (0, 3, 4, 9, 12, 17), lines, trace_only=args.trace_only)
    if args.trace_only:
        return
    lines.append("")
    writer_report(*titan, (0, 3, 4, 9, 12, 17), lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
