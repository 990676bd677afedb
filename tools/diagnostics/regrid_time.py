"""Times the regrid of native-grid planes on the device (datapipe.load_native_batch -> p4c_regrid_pack) at the Titan training
shape -- B = 2, T = 4, the sub-domain [100:612, 240:880] (512 x 640) of PAAROME_1S100 (1791 x 2801), 21 features: 13 from
PAAROME_1S40 planes (717 x 1121) and 8 from the 180 x 281 AROME window of PA_01D planes (521 x 741) -- and in the same process
the device sequence it replaces, built from library operations: F.interpolate(mode="bilinear", align_corners=False) to the full
grid (the same coordinate map; it differs at the border only and stands here for time, not for parity), flip, slice,
ops.pack_standardize.  Also the down-sampling direction (PAAROME_1S100 planes -> PAAROME_1S40 with the Gaussian), the end to end
time with the pinned upload of the source planes, and one plane through the scipy.ndimage form on the host.

    python tools/diagnostics/regrid_time.py [--out profiles/regrid.txt]

Kernel and call times: device events around n calls, median (and range) of 7 windows after warm-up calls.  End to end: host clock
around one call ending in a synchronise, median of 10 after 3 warm-up calls."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from py4cast_amd import datapipe, ops, regrid  # noqa: E402

PEAK_TBS = 8.0
dev = torch.device("cuda:0")
FULL, FULL40, SUB = (1791, 2801), (717, 1121), (100, 612, 240, 880)
ARP_SHAPE, ARP_WINDOW = (521, 741), (166, 346, 200, 481)


def device_windows(fn, n, windows=7, warm=5):
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
    return out


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


def fmt(w):
    return f"{statistics.median(w):9.1f} us   (7 windows: {min(w):.1f} .. {max(w):.1f})"


class Stats:
    def __init__(self, n):
        self.d = {"mean": torch.linspace(-1, 1, n), "std": torch.linspace(0.5, 2, n)}

    def to_list(self, stat, names, dtype=torch.float32):
        return self.d[stat].type(dtype)


def library_sequence(groups, io_names, mean, std):
    """interpolate to the full grid, flip, slice, pack: what the fused call replaces, from library operations"""
    planes = {}
    a, b, c, d = SUB
    for raw, names, plan in groups:
        r0, r1, c0, c1 = plan.window
        Fg, B, T = raw.shape[:3]
        full = F.interpolate(raw[..., r0:r1, c0:c1].reshape(Fg, B * T, r1 - r0, c1 - c0), size=plan.full_size, mode="bilinear",
                             align_corners=False)
        cut = full.flip(-2)[..., a:b, c:d].reshape(Fg, B, T, b - a, d - c)
        planes.update({n: cut[k] for k, n in enumerate(names)})
    return ops.pack_standardize(torch.stack([planes[n] for n in io_names]), mean, std)


def titan_training(lines):
    B, T = 2, 4
    aro = regrid.RegridPlan(FULL40, FULL, subdomain=SUB)
    arp = regrid.RegridPlan(ARP_SHAPE, FULL, window=ARP_WINDOW, subdomain=SUB)
    g = torch.Generator().manual_seed(1)
    host = [torch.randn(13, B, T, *FULL40, generator=g).pin_memory(), torch.randn(8, B, T, *ARP_SHAPE, generator=g).pin_memory()]
    names = [[f"aro{i}" for i in range(13)], [f"arp{i}" for i in range(8)]]
    io_names = [n for pair in zip(names[0], names[1] + [None] * 5) for n in pair if n]        # interleaved
    stats = Stats(21)
    mean, std = stats.d["mean"].to(dev), stats.d["std"].to(dev)
    groups = [(h.to(dev), ns, p) for h, ns, p in zip(host, names, (aro, arp))]
    Hs, Ws = aro.out_shape
    rows = B * T * Hs * Ws
    out_bytes = 4 * rows * 21
    src_bytes = regrid.source_bytes(aro, 13 * B * T) + regrid.source_bytes(arp, 8 * B * T)
    alg = src_bytes + out_bytes

    fused = datapipe.load_native_batch(groups, io_names, None, stats, T)
    lib = library_sequence(groups, io_names, mean, std)
    diff = (fused.inputs.tensor - lib).abs().max().item()

    # the kernel alone: descriptors and tables already on the device
    sources = [g[0] for g in groups]
    feats = []
    for c, n in enumerate(io_names):
        gi = 0 if n.startswith("aro") else 1
        plan = groups[gi][2]
        feats.append((gi, names[gi].index(n), plan.window[0], plan.window[2], gi, float(stats.d["mean"][c]), float(stats.d["std"][c]), c))
    feats.sort(key=lambda f: (f[4], f[0], f[1]))
    dims = [aro.n, arp.n]
    feats_dev, taps = ops.regrid_features(sources, feats, dims, B, T), regrid.device_taps([aro, arp], dev)
    assert torch.equal(ops.regrid_pack(sources, feats_dev, taps, dims, B, T, Hs, Ws), fused.inputs.tensor)
    k_w = device_windows(lambda: ops.regrid_pack(sources, feats_dev, taps, dims, B, T, Hs, Ws), n=50)
    f_w = device_windows(lambda: datapipe.load_native_batch(groups, io_names, None, stats, T), n=50)
    l_w = device_windows(lambda: library_sequence(groups, io_names, mean, std), n=5, warm=2)
    raw_p = torch.randn(21, B, T, Hs, Ws, device=dev)
    p_w = device_windows(lambda: ops.pack_standardize(raw_p, mean, std), n=50)
    e_us = wall_us(lambda: datapipe.load_native_batch(groups, io_names, None, stats, T))
    u_us = wall_us(lambda: datapipe.load_native_batch([(h.to(dev, non_blocking=True), ns, p) for h, ns, p in zip(host, names, (aro, arp))],
                                                      io_names, None, stats, T))
    up_bytes = sum(h.numel() * 4 for h in host)

    k_us = statistics.median(k_w)
    lines.append(f"Titan training shape: B={B} T={T}, sub-domain {Hs} x {Ws} of {FULL[0]} x {FULL[1]}, 21 features = 13 from {FULL40[0]} x {FULL40[1]} planes + 8 "
                 f"from the {arp.n[0]} x {arp.n[1]} window of {ARP_SHAPE[0]} x {ARP_SHAPE[1]} planes; output {out_bytes / 1e6:.1f} MB, source footprint {src_bytes / 1e6:.1f} MB")
    lines.append(f"  p4c_regrid_pack (kernel, descriptors on the device)   {fmt(k_w)}   {alg / k_us / 1e6:5.2f} TB/s of {alg / 1e6:.1f} MB algorithmic"
                 f" = {100 * alg / k_us / 1e6 / PEAK_TBS:4.1f}% of {PEAK_TBS:.0f} TB/s")
    lines.append(f"  datapipe.load_native_batch (the fused call)           {fmt(f_w)}")
    lines.append(f"  library sequence: interpolate, flip, slice, pack      {fmt(l_w)}")
    lines.append(f"  ops.pack_standardize, 21 planes, same output bytes    {fmt(p_w)}")
    lines.append(f"  load_native_batch end to end, planes on the device    {e_us:9.1f} us   host clock to a synchronise")
    lines.append(f"  the same with the pinned upload of the planes         {u_us:9.1f} us   {up_bytes / 1e6:.0f} MB uploaded")
    ok = max(f_w) < min(l_w)
    lines.append(f"  condition (slowest fused window < fastest library window): {max(f_w):.1f} < {min(l_w):.1f} us: {'MET' if ok else 'NOT MET'}"
                 f"; library / fused = x{statistics.median(l_w) / statistics.median(f_w):.1f}")
    lines.append(f"  fused against the library sequence on the (interior) sub-domain: max |difference| {diff:.3g} (standardised values)")
    return host[0][0, 0, 0].numpy()


def titan_downsampling(lines):
    """PAAROME_1S100 planes onto PAAROME_1S40 with the Gaussian (sigma 0.749, radius 3): one blur launch, then the pack"""
    B, T, Fg = 2, 4, 3
    sub = (100, 612, 240, 880)
    plan = regrid.RegridPlan(FULL, FULL40, subdomain=sub, anti_aliasing=True)
    raw = torch.randn(Fg, B, T, *FULL, device=dev)
    names, stats = [f"p{i}" for i in range(Fg)], Stats(Fg)
    tables = regrid.device_blur_tables(plan, dev)
    b_w = device_windows(lambda: ops.regrid_blur(raw, plan.window, *tables), n=10, warm=2)
    f_w = device_windows(lambda: datapipe.load_native_batch([(raw, names, plan)], names, None, stats, T), n=10, warm=2)
    b_us, planes = statistics.median(b_w), Fg * B * T
    alg = 4 * planes * 2 * FULL[0] * FULL[1]
    lines.append(f"down-sampling with the blur: {Fg} features, B={B} T={T}, {FULL[0]} x {FULL[1]} -> {FULL40[0]} x {FULL40[1]}, sub-domain {plan.out_shape[0]} x {plan.out_shape[1]}, "
                 f"sigma {plan.sigma[0]:.3f}, radius {plan.radius[0]}")
    lines.append(f"  p4c_regrid_blur ({planes} whole planes)                   {fmt(b_w)}   {alg / b_us / 1e6:5.2f} TB/s of {alg / 1e6:.1f} MB algorithmic"
                 f" = {100 * alg / b_us / 1e6 / PEAK_TBS:4.1f}% of {PEAK_TBS:.0f} TB/s")
    lines.append(f"  datapipe.load_native_batch (blur + pack)              {fmt(f_w)}")


def host_plane(plane, lines):
    try:
        from scipy import ndimage as ndi
    except ImportError:
        lines.append("one plane on the host: scipy is not installed, not measured")
        return
    img = plane.astype(np.float64)
    factors = np.array(img.shape) / np.array(FULL, dtype=np.float64)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        ndi.zoom(img, 1 / factors, order=1, mode="mirror", grid_mode=True)[::-1][SUB[0]:SUB[1], SUB[2]:SUB[3]]
        times.append((time.perf_counter() - t0) * 1e6)
    lines.append(f"one {img.shape[0]} x {img.shape[1]} plane through scipy.ndimage.zoom to {FULL[0]} x {FULL[1]} on the host (float64): "
                 f"{statistics.median(times) / 1e3:.1f} ms; the training shape has {21 * 2 * 4} planes per batch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "regrid.txt"))
    args = ap.parse_args()
    lines = [f"regrid of native-grid planes on the device: tools/diagnostics/regrid_time.py on {torch.cuda.get_device_name(0)}",
             "device events, median and range of 7 windows (50 calls; 5 for the library sequence, 10 with the blur); end to end: host clock to a "
             "synchronise, median of 10", ""]
    plane = titan_training(lines)
    lines.append("")
    titan_downsampling(lines)
    lines.append("")
    host_plane(plane, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
