"""Times reading complex-packed GRIB2 fields (template 5.3, order 2) on the device -- one pinned copy of the section-7 payloads of a
batch and ops.grib_unpack_complex -- against the two yardsticks of profiles/grib_unpack.txt: the pinned copy of the same fields as
fp32 planes alone (the floor of any host decoder) and the 5.0 decode, ops.grib_unpack, of the same integers at 16 bits.

    python tools/diagnostics/grib_complex_time.py [--out profiles/grib_complex.txt]

Input: a smooth synthetic field (a few waves across the grid) plus noise of about two units, quantised to 16-bit integers as a
D-scaled field would be, encoded at order 2 in groups of 32 values by the encoder of tests/grib_complex_cases.py.  A few distinct
fields are encoded and repeated over the batch (the encoder is a Python loop); every repeat has its own copy of the stream in the
buffer.  The bits per value reached are a property of this synthetic field, not of real data.

Clocks: host clock around one call ending in a synchronise, 3 alternating rounds of 10 native (payload copy + decode) / 3 fp32-copy
calls after warm-up calls, median of the rounds' medians; the decode calls alone also with device events (median of 7 windows of 20
calls).  The launches of a call are told apart by a kernel trace of this script (``rocprofv3 --kernel-trace --stats -- python
tools/diagnostics/grib_complex_time.py --trace-only``: a run of its own, the averages go into the file by hand)."""
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
import grib_complex_cases as cc  # noqa: E402
import grib_unpack_cases as cases  # noqa: E402
from py4cast_amd import grib2, ops  # noqa: E402

dev = torch.device("cuda:0")
E, D, GROUP, DISTINCT = -4, 2, 32, 3


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


def synthetic(g, nj, ni):
    """16-bit integers of a smooth field plus noise, stream order"""
    y, x = np.mgrid[0:nj, 0:ni]
    smooth = 30000 + 12000 * np.sin(x / ni * 5.1 + g.random() * 6) * np.cos(y / nj * 3.7 + g.random() * 6) + 9000 * np.sin((x + 2 * y) / (ni + nj) * 9.0)
    return np.clip(np.rint(smooth + g.normal(0.0, 2.0, size=smooth.shape)), 0, 65535).astype(np.int64).reshape(-1)


def batch(fields, nj, ni, g):
    """`fields` complex-packed fields (DISTINCT different ones, repeated) and the same integers simple-packed at 16 bits, each set in
    a pinned byte buffer of its own -> (complex buffer, GRIB_CFIELD table, simple buffer, GRIB_FIELD table, the integers)"""
    N = ni * nj
    pitch = (N + 3) // 4 * 4
    integers, payloads, records, simple = [], [], [], []
    for i in range(DISTINCT):
        f = synthetic(g, nj, ni)
        msg = cc.message(ni, nj, f, 2, list(range(0, N, GROUP)), 250.0, E, D, nbytes=3, l_ref=GROUP, l_bits=0, w_bits=5, ref_bits=16)
        field = grib2.complex_field_of(msg)
        integers.append(f)
        payloads.append(np.frombuffer(bytes(field.stream), dtype=np.uint8))
        records.append(field)
        simple.append(np.frombuffer(cases.stream_of(f.astype(np.uint64), 16), dtype=np.uint8))
    ctable = np.zeros(fields, dtype=ops.GRIB_CFIELD)
    table = np.zeros(fields, dtype=ops.GRIB_FIELD)
    at = at16 = 0
    for i in range(fields):
        f, payload, stream = records[i % DISTINCT], payloads[i % DISTINCT], simple[i % DISTINCT]
        rec = ctable[i]
        rec["stream_off"], rec["stream_len"], rec["bitmap_off"], rec["dst_off"] = at, payload.size, -1, i * pitch
        for name in ("ni", "nj", "count", "ng", "ref_bits", "w_ref", "w_bits", "l_ref", "l_inc", "l_last", "l_bits", "order", "nbytes", "ival1",
                     "ival2", "gmin", "E", "D", "R"):
            rec[name] = getattr(f, name)
        table[i] = (at16, stream.size, -1, i * pitch, ni, nj, N, 16, E, D, 250.0, 0, 0, 0)
        at += (payload.size + 3) // 4 * 4
        at16 += (stream.size + 3) // 4 * 4
    host, host16 = torch.empty(at, dtype=torch.uint8, pin_memory=True), torch.empty(at16, dtype=torch.uint8, pin_memory=True)
    for i in range(fields):
        host.numpy()[ctable[i]["stream_off"]:][:ctable[i]["stream_len"]] = payloads[i % DISTINCT]
        host16.numpy()[table[i]["stream_off"]:][:table[i]["stream_len"]] = simple[i % DISTINCT]
    return host, ctable, host16, table, integers


def shape_report(title, B, T, nj, ni, F, lines, rounds=3, trace_only=False):
    fields, N = B * T * F, nj * ni
    g = np.random.default_rng(0)
    host, ctable, host16, table, integers = batch(fields, nj, ni, g)
    pitch = (N + 3) // 4 * 4
    planes = torch.empty(fields * pitch, dtype=torch.float32, device=dev)
    status = torch.empty(fields, dtype=torch.int32, device=dev)
    packed, packed16 = host.to(dev), host16.to(dev)

    def unpack():
        return ops.grib_unpack_complex(packed, ctable, out=planes, status=status)

    def unpack16():
        return ops.grib_unpack(packed16, table, out=planes)

    def native():
        ops.grib_unpack_complex(host.to(dev, non_blocking=True), ctable, out=planes, status=status)

    if trace_only:
        for fn in (unpack, unpack16):
            for _ in range(25):
                fn()
        torch.cuda.synchronize()
        return
    host32 = torch.empty(fields * N, dtype=torch.float32, pin_memory=True)

    def fp32_copy():
        return host32.to(dev, non_blocking=True)

    wall_us(native, n=3), wall_us(fp32_copy, n=2)
    nat, old = [], []
    for _ in range(rounds):
        nat.append(wall_us(native, n=10))
        old.append(wall_us(fp32_copy, n=3))
    n_us, o_us = statistics.median(nat), statistics.median(old)
    c_us = wall_us(lambda: host.to(dev, non_blocking=True), n=10, warm=3)
    u_us = wall_us(unpack, n=10, warm=3)
    d16_us = device_us(unpack16)
    d_us = device_us(unpack)
    assert not status.cpu().numpy().any()
    for i in range(DISTINCT):                       # the decoded planes are the integers that went in, bit for bit
        got = planes[i * pitch:i * pitch + N].cpu().numpy()
        assert cases.same_bits(got, cc.expected_plane(integers[i], ni, nj, 250.0, E, D).reshape(-1)), f"{title}: field {i} differs"
    streams, streams16 = int(ctable["stream_len"].sum()), int(table["stream_len"].sum())
    lines.append(f"{title}: {B}x{T}x{nj}x{ni}x{F} = {fields} fields of {N} points, order 2, groups of {GROUP} values: payloads {streams / 1e6:.1f} MB "
                 f"= {8 * streams / (fields * N):.2f} bits per value (16-bit streams {streams16 / 1e6:.1f} MB), fp32 planes {4 * fields * N / 1e6:.1f} MB")
    lines.append(f"  payload copy + grib_unpack_complex, host clock to a synchronise   {n_us:10.1f} us   (rounds {' '.join(f'{v:.0f}' for v in nat)})")
    lines.append(f"    of which the pinned copy of the payloads, same clock            {c_us:10.1f} us   {streams / c_us / 1e3:5.1f} GB/s")
    lines.append(f"    and the grib_unpack_complex call alone, same clock              {u_us:10.1f} us")
    lines.append(f"  yardstick 1: pinned copy of the fp32 planes alone, host clock     {o_us:10.1f} us   {4 * fields * N / o_us / 1e3:5.1f} GB/s   "
                 f"(rounds {' '.join(f'{v:.0f}' for v in old)})   ratio to the payload copy + decode {o_us / n_us:.2f}")
    lines.append(f"  grib_unpack_complex, device events (4 launches: sums, scan, tiles, decode) {d_us:10.1f} us")
    lines.append(f"  yardstick 2: grib_unpack of the same integers at 16 bits, device events (1 launch) {d16_us:10.1f} us   "
                 f"ratio complex / simple {d_us / d16_us:.2f}")
    lines.append(f"  the {DISTINCT} distinct fields equal float32((R + ldexp(f, E)) / 10^D) of their integers bit for bit; every status word is 0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "grib_complex.txt"))
    ap.add_argument("--trace-only", action="store_true", help="only 25 decode calls of either kind per case, for a kernel trace")
    args = ap.parse_args()
    lines = [f"GRIB2 complex packing (5.3, order 2) decoded on the device: tools/diagnostics/grib_complex_time.py on {torch.cuda.get_device_name(0)}",
             "host clock around one call ending in a synchronise, 3 alternating rounds of 10 / 3 calls, median of the rounds' medians; the "
             "decode calls also with device events, median of 7 windows of 20 calls", ""]
    for title, shape in (("PAAROME_1S40, 2 input + 3 target steps", (2, 5, 717, 1121, 21)), ("benchmark shape", (2, 5, 512, 512, 60))):
        shape_report(title, *shape, lines, trace_only=args.trace_only)
        lines.append("")
        torch.cuda.empty_cache()
    if args.trace_only:
        return
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
