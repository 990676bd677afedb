"""Times reading GRIB2 fields on the device -- one pinned copy of the packed bit streams (and bitmaps) of a batch and ops.grib_unpack --
against what the package could do with the same messages before: ``grib2.decode`` per field on the host, ``.astype(float32)``, one
pinned copy of the fp32 planes.  The two halves of that older route are reported separately: the copy alone is the floor a better
host decoder could reach.  The reference's own host decode (cfgrib / eccodes, datasets/titan/__init__.py:112-152) cannot be timed
here: neither library is installed; it is OUTSIDE the comparison.

    python tools/diagnostics/grib_unpack_time.py [--out profiles/grib_unpack.txt]

Clocks: host clock around one call ending in a synchronise, 3 alternating rounds of 10 native (packed copy + unpack) / 3 older-route
(fp32 copy) calls after warm-up calls, median of the rounds' medians; the unpack call alone also with device events (median of 7
windows of 20 calls).  ``grib2.decode`` is timed on a few fields of the shape (host clock, median) and multiplied by the number of
fields: decoding all of them takes minutes.  The launches of a call with bitmaps are told apart by a kernel trace of this script
(``rocprofv3 --kernel-trace --stats -- python tools/diagnostics/grib_unpack_time.py --trace-only``: a run of its own, the averages go
into the file by hand).  Bytes moved by the unpack call: streams and bitmaps read once (the count launch reads the bitmaps once
more), planes written."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grib_unpack_cases as cases  # noqa: E402
from py4cast_amd import grib2, ops  # noqa: E402

dev = torch.device("cuda:0")
NBITS, E, D = 16, -4, 2


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


def batch(fields, nj, ni, density, g):
    """random 16-bit streams (and bitmaps of the given density) of `fields` fields in one pinned byte buffer -> (buffer, table, the
    bitmaps as bool arrays or None)"""
    N = ni * nj
    table = np.zeros(fields, dtype=ops.GRIB_FIELD)
    chunks, at, presents = [], 0, []
    for i in range(fields):
        present = (g.random(N) < density) if density is not None else None
        count = N if present is None else int(present.sum())
        stream = g.integers(0, 256, size=(count * NBITS + 7) // 8, dtype=np.uint8)
        s_off, b_off = at, -1
        chunks.append((at, stream))
        at += (stream.size + 3) // 4 * 4
        if present is not None:
            bitmap = np.packbits(present)
            b_off = at
            chunks.append((at, bitmap))
            at += (bitmap.size + 3) // 4 * 4
        presents.append(present)
        table[i] = (s_off, stream.size, b_off, i * ((N + 3) // 4 * 4), ni, nj, count, NBITS, E, D, 250.0 + i, 0, 0, 0)
    host = torch.empty(at, dtype=torch.uint8, pin_memory=True)
    view = host.numpy()
    for off, data in chunks:
        view[off:off + data.size] = data
    return host, table, presents


def shape_report(title, B, T, nj, ni, F, density, lines, rounds=3, trace_only=False, sampled=3):
    fields, N = B * T * F, nj * ni
    g = np.random.default_rng(0)
    host, table, presents = batch(fields, nj, ni, density, g)
    pitch = (N + 3) // 4 * 4
    planes = torch.empty(fields * pitch, dtype=torch.float32, device=dev)
    packed = host.to(dev)

    def unpack():
        return ops.grib_unpack(packed, table, out=planes)

    def native():
        ops.grib_unpack(host.to(dev, non_blocking=True), table, out=planes)

    if trace_only:
        for _ in range(25):
            unpack()
        torch.cuda.synchronize()
        return
    host32 = torch.empty(fields * N, dtype=torch.float32, pin_memory=True)

    def older_copy():
        return host32.to(dev, non_blocking=True)

    wall_us(native, n=3), wall_us(older_copy, n=2)
    nat, old = [], []
    for _ in range(rounds):
        nat.append(wall_us(native, n=10))
        old.append(wall_us(older_copy, n=3))
    n_us, o_us = statistics.median(nat), statistics.median(old)
    c_us = wall_us(lambda: host.to(dev, non_blocking=True), n=10, warm=3)
    u_us = wall_us(unpack, n=10, warm=3)
    d_us = device_us(unpack)
    # the older route's host half on a few fields: the very messages, through grib2.decode
    view, dec = host.numpy(), []
    for i in range(sampled):
        rec = table[i]
        X = grib2.unpack_bits(view[rec["stream_off"]:rec["stream_off"] + rec["stream_len"]].tobytes(), int(rec["count"]), NBITS)
        msg = grib2.Message(cases.message(ni, nj, X, NBITS, float(rec["R"]), E, D, present=presents[i]))
        t0 = time.perf_counter()
        plane = grib2.decode(msg)[0].filled(np.nan).astype(np.float32)
        dec.append((time.perf_counter() - t0) * 1e6)
        a = int(rec["dst_off"])
        got = planes[a:a + N].cpu().numpy()
        assert cases.same_bits(got, plane.reshape(-1)), f"{title}: field {i} differs from grib2.decode"
    h_us = statistics.median(dec)
    streams = int(table["stream_len"].sum())
    bitmaps = 0 if density is None else fields * ((N + 7) // 8)
    moved = streams + bitmaps + 4 * fields * N
    what = "no bitmap" if density is None else f"bitmaps of density {density}"
    lines.append(f"{title}: {B}x{T}x{nj}x{ni}x{F} = {fields} fields of {N} points, {NBITS} bits, {what}: streams {streams / 1e6:.1f} MB, "
                 f"bitmaps {bitmaps / 1e6:.1f} MB, fp32 planes {4 * fields * N / 1e6:.1f} MB")
    lines.append(f"  packed copy + grib_unpack, host clock to a synchronise          {n_us:10.1f} us   (rounds {' '.join(f'{v:.0f}' for v in nat)})")
    lines.append(f"    of which the pinned copy of streams + bitmaps, same clock     {c_us:10.1f} us   {(streams + bitmaps) / c_us / 1e3:5.1f} GB/s")
    lines.append(f"    and the grib_unpack call alone, same clock                    {u_us:10.1f} us")
    lines.append(f"  grib_unpack, device events ({'1 launch' if density is None else 'count + unpack launches'})"
                 f"{'':>{22 if density is None else 7}}{d_us:10.1f} us   {moved / d_us / 1e6:5.2f} TB/s of streams + bitmaps read and planes written "
                 f"({moved / 1e6:.1f} MB)")
    lines.append(f"  older route, copy half: pinned copy of the fp32 planes, host clock {o_us:10.1f} us   {4 * fields * N / o_us / 1e3:5.1f} GB/s   "
                 f"(rounds {' '.join(f'{v:.0f}' for v in old)})   ratio to the packed copy + unpack {o_us / n_us:.2f}")
    lines.append(f"  older route, decode half: grib2.decode + astype(float32), host clock, median of {sampled} fields {h_us:10.1f} us per field, "
                 f"x {fields} fields = {h_us * fields / 1e6:.2f} s   ratio of both halves to the packed copy + unpack {(h_us * fields + o_us) / n_us:.0f}")
    lines.append(f"  the {sampled} decoded fields equal the device planes bit for bit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "grib_unpack.txt"))
    ap.add_argument("--trace-only", action="store_true", help="only 25 unpack calls per case, for a kernel trace")
    args = ap.parse_args()
    lines = [f"GRIB2 simple packing decoded on the device: tools/diagnostics/grib_unpack_time.py on {torch.cuda.get_device_name(0)}",
             "host clock around one call ending in a synchronise, 3 alternating rounds of 10 / 3 calls, median of the rounds' medians; the "
             "unpack call also with device events, median of 7 windows of 20 calls; grib2.decode on 3 fields per case", ""]
    for title, shape in (("PAAROME_1S40, 2 input + 3 target steps", (2, 5, 717, 1121, 21)), ("benchmark shape", (2, 5, 512, 512, 60))):
        for density in (None, 0.5):
            shape_report(title, *shape, density, lines, trace_only=args.trace_only)
            lines.append("")
            torch.cuda.empty_cache()
    if args.trace_only:
        return
    lines.append("not measured: the reference's host decode (cfgrib / eccodes): neither library is installed on these machines.")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
