"""Times the forcing batch built on the device (datapipe.build_forcing -> p4c_build_forcing) at the benchmark's forcing shape
(2 x 3 x 512^2, no external planes) and the Titan shape (2 x 1 x 512 x 640, 16 external planes), and in the same process what it
stands beside: ops.pack_standardize at the same output bytes, a pinned host-to-device copy of the same tensor (what it replaces)
and the host generation in float64 (forcings.host_forcing: the reference assembles these channels per sample on the CPU).

    python tools/diagnostics/forcing_time.py [--out profiles/forcing_build.txt]

Kernel times: device events around 50 calls, median of 7 windows after 10 warm-up calls.  End-to-end times (host tables, their
upload, the launch): host clock around one call ending in a synchronise, median of 30 after 5 warm-up calls."""
import argparse
import datetime as dt
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from py4cast_amd import datapipe, forcings, ops  # noqa: E402

PEAK_TBS = 8.0
dev = torch.device("cuda:0")


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


def wall_us(fn, n=30, warm=5, sync=True):
    out = []
    for i in range(warm + n):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


class Stats:
    def __init__(self, n):
        self.d = {"mean": torch.linspace(-1, 1, n), "std": torch.linspace(0.5, 2, n)}

    def to_list(self, stat, names, dtype=torch.float32):
        return self.d[stat].type(dtype)


def shape_report(title, B, T, H, W, Fe, lines):
    lat, lon = np.meshgrid(np.linspace(55, 37, H, dtype=np.float32), np.linspace(-12, 16, W, dtype=np.float32), indexing="ij")
    dates = [dt.datetime(2023, 3, 20, 11, 15) + dt.timedelta(days=30 * b) for b in range(B)]
    terms = [dt.timedelta(hours=1 + t) for t in range(T)]
    rows, F = B * T * H * W, Fe + 5
    raw = torch.randn(Fe, B, T, H, W, device=dev) if Fe else None
    names, stats = [f"e{i}" for i in range(Fe)], Stats(Fe)
    mean, std = (stats.d["mean"].to(dev), stats.d["std"].to(dev)) if Fe else (None, None)
    table, planes = forcings.time_table(dates, terms).to(dev), forcings.grid_tables(lat, lon, dev)
    out = datapipe.build_forcing(raw, names, stats, dates, terms, lat, lon, device=dev)
    alg, out_bytes = 4 * rows * (2 * Fe + 5), 4 * rows * F

    k_us = device_us(lambda: ops.build_forcing(raw, mean, std, table, planes, B, T, H, W))
    e_us = wall_us(lambda: datapipe.build_forcing(raw, names, stats, dates, terms, lat, lon, device=dev))
    raw_p = torch.randn(F, B, T, H, W, device=dev)
    mp, sp = torch.zeros(F, device=dev), torch.ones(F, device=dev)
    p_us = device_us(lambda: ops.pack_standardize(raw_p, mp, sp))
    pinned = out.tensor.cpu().pin_memory()
    dst = torch.empty_like(out.tensor)
    c_us = wall_us(lambda: dst.copy_(pinned, non_blocking=True))
    h_us = wall_us(lambda: forcings.host_forcing(dates, terms, lat, lon), n=5, warm=1, sync=False)

    lines.append(f"{title}: B={B} T={T} H={H} W={W}, {Fe} external + 5 generated features, output {out_bytes / 1e6:.1f} MB")
    lines.append(f"  p4c_build_forcing (kernel, tables on the device)    {k_us:9.1f} us   {alg / k_us / 1e6:5.2f} TB/s of {alg / 1e6:.1f} MB algorithmic"
                 f" = {100 * alg / k_us / 1e6 / PEAK_TBS:4.1f}% of {PEAK_TBS:.0f} TB/s")
    lines.append(f"  datapipe.build_forcing (host tables + upload + kernel) {e_us:6.1f} us   end to end, synchronised")
    lines.append(f"  ops.pack_standardize, {F} planes, same output bytes  {p_us:9.1f} us   {2 * out_bytes / p_us / 1e6:5.2f} TB/s of {2 * out_bytes / 1e6:.1f} MB algorithmic")
    lines.append(f"  pinned host-to-device copy of the same tensor       {c_us:9.1f} us   {out_bytes / c_us / 1e3:5.1f} GB/s")
    lines.append(f"  host generation of the 5 channels (float64, torch)  {h_us:9.1f} us   (before any copy)")
    lines.append(f"  end to end against the pinned copy: x{c_us / e_us:.1f}; against host generation + copy: x{(h_us + c_us) / e_us:.1f}")
    return k_us, e_us, c_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "forcing_build.txt"))
    args = ap.parse_args()
    lines = [f"forcing batch on the device: tools/diagnostics/forcing_time.py on {torch.cuda.get_device_name(0)}",
             "kernel: device events, median of 7 windows of 50 calls; end to end and copy: host clock to a synchronise, median of 30", ""]
    shape_report("benchmark forcing", 2, 3, 512, 512, 0, lines)
    lines.append("")
    shape_report("Titan forcing", 2, 1, 512, 640, 16, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
