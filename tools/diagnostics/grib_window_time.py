"""Times the two routes from simple-packed GRIB2 fields that are already on the target grid to the standardised features-last batch on
the sub-domain, at the Titan shape: 2 x 5 x 717 x 1121 x 21 at 16 bits, sub-domain [100, 612, 240, 880], messages synthesised with
``grib2.encode`` around random bit streams.

    window route      the pinned copy of the slices that hold the sub-domain's rows (``grib2.window_slice``) and ONE launch,
                      ``p4c_grib_window_pack`` (``datapipe.load_window_batch``);
    two-launch route  the pinned copy of the whole streams, ``p4c_grib_unpack`` into fp32 native planes and ``p4c_regrid_pack`` through
                      the identity plan (``datapipe.load_native_batch``): the route of ``diskio.load_titan_grib_batch``.

    python tools/diagnostics/grib_window_time.py [--out profiles/grib_window.txt]

Clocks: host clock around one call ending in a synchronise, 3 alternating rounds of 10 calls of each route after warm-up calls,
median of the rounds' medians; the launches alone with device events (median of 7 windows of 20 calls).  Loader: ``DeviceLoader``
over a tree of 8 dates (4 samples, batches of 2) whose files are in the page cache, ``GribRoutes.use_window`` on and off in
5 alternating rounds of 3 epochs after one warm-up epoch each, batches per second of the host clock from the first ``next`` to a
synchronise after the last batch; 8 reader threads, prefetch 2.  The warm-up epoch parses all files into the loader's index, so the
figure holds no parsing: an index that is not in the cache (a shuffled order, an archive of more files than the cache keeps) is NOT
measured.  The device-event figures are taken around the Python call, which also uploads the descriptor table; they are not a kernel
trace.  The outputs of the two routes are compared bit for bit."""
import argparse
import datetime as dt
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grib_window_cases as wc  # noqa: E402
from py4cast_amd import datapipe, datasets, diskio, grib2, ops, regrid  # noqa: E402

dev = torch.device("cuda:0")
B, T, NJ, NI, F = 2, 5, 717, 1121, 21
SUB = (100, 612, 240, 880)
LEVELS = [1000 - 25 * i for i in range(F)]
E, D = -4, 2


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


def messages(g, dates):
    """per date the bytes of one file: F messages (one per level) made by ``grib2.encode`` around a random 16-bit stream"""
    templates = [grib2.Message(wc._grid_message(g, NJ, NI, 55.4, -12.0, 0.025, 16, 0, 0, 100, level)) for level in LEVELS]
    out = []
    for date in dates:
        parts = []
        for f, tmpl in enumerate(templates):
            packed = g.integers(0, 256, size=NJ * NI * 2, dtype=np.uint8).tobytes()
            parts.append(grib2.encode(tmpl, date, dt.timedelta(0), window=(0, NJ - 1, 0, NI - 1), packed=packed, R=250.0 + f, E=E, D=D, nbits=16))
        out.append(b"".join(parts))
    return out


def device_routes(files, lines):
    plan = regrid.RegridPlan((NJ, NI), (NJ, NI), subdomain=SUB)
    rows = datapipe.window_rows(plan)
    names = [f"f{f}" for f in range(F)]
    parsed = [grib2.parse_messages(data) for data in files]                       # date -> its F messages
    fields = [[[grib2.field_of(parsed[b + t][f]) for t in range(T)] for b in range(B)] for f in range(F)]
    # the slices and the whole streams, each message once, in two pinned buffers
    s_place, w_place, s_at, w_at = {}, {}, 0, 0
    for f in range(F):
        for b in range(B):
            for t in range(T):
                key = (b + t, f)
                if key not in s_place:
                    first, end, bit0 = grib2.window_slice(fields[f][b][t], *rows)
                    s_place[key] = (s_at, end - first, bit0, first)
                    s_at += (end - first + 3) // 4 * 4
                    w_place[key] = w_at
                    w_at += (len(fields[f][b][t].stream) + 3) // 4 * 4
    host_s = torch.empty(s_at, dtype=torch.uint8, pin_memory=True)
    host_w = torch.empty(w_at, dtype=torch.uint8, pin_memory=True)
    for (d, f), (off, n, _, first) in s_place.items():
        stream = np.frombuffer(grib2.field_of(parsed[d][f]).stream, dtype=np.uint8)
        host_s.numpy()[off:off + n] = stream[first:first + n]
        host_w.numpy()[w_place[d, f]:w_place[d, f] + stream.size] = stream
    places = [[[s_place[b + t, f][:3] for t in range(T)] for b in range(B)] for f in range(F)]
    table = datapipe.window_table(fields, places, names, plan)
    g = np.random.default_rng(1)
    stats = wc.Stats({n: (float(np.float32(250 + g.normal())), float(np.float32(1 + g.random()))) for n in names})
    pitch = (NJ * NI + 3) // 4 * 4
    chosen = [("", None, fields[f][b][t]) for f in range(F) for b in range(B) for t in range(T)]
    where = [(w_place[b + t, f], -1) for f in range(F) for b in range(B) for t in range(T)]

    def window_launch(buf):
        return datapipe.load_window_batch(buf, table, names, None, stats, T).inputs.tensor

    def two_launches(buf):
        flat, _ = diskio.decode_placed(buf, chosen, where, pitch)
        planes = flat.as_strided((F, B, T, NJ, NI), (B * T * pitch, T * pitch, pitch, NI, 1))
        return datapipe.load_native_batch([(planes, names, plan)], names, None, stats, T).inputs.tensor

    dev_s, dev_w = host_s.to(dev), host_w.to(dev)
    a, b = window_launch(dev_s), two_launches(dev_w)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(torch.isfinite(a).all()), "the two routes differ"
    del a, b
    route_w = lambda: window_launch(host_s.to(dev, non_blocking=True))      # noqa: E731
    route_t = lambda: two_launches(host_w.to(dev, non_blocking=True))       # noqa: E731
    wall_us(route_w, n=3), wall_us(route_t, n=3)
    win, two = [], []
    for _ in range(3):
        win.append(wall_us(route_w, n=10))
        two.append(wall_us(route_t, n=10))
    w_us, t_us = statistics.median(win), statistics.median(two)
    cw_us = wall_us(lambda: host_s.to(dev, non_blocking=True), n=10, warm=3)
    ct_us = wall_us(lambda: host_w.to(dev, non_blocking=True), n=10, warm=3)
    kw_us = device_us(lambda: window_launch(dev_s))
    kt_us = device_us(lambda: two_launches(dev_w))
    H, W = plan.out_shape
    out_bytes = 4 * B * T * H * W * F
    read = 2 * B * T * H * W * F
    lines.append(f"{B}x{T}x{NJ}x{NI}x{F} = {B * T * F} fields ({len(s_place)} distinct messages) of 16 bits, sub-domain {list(SUB)} = {H} x {W}: "
                 f"batch {out_bytes / 1e6:.1f} MB")
    lines.append(f"  bytes copied: window route {s_at / 1e6:.1f} MB of slices ({rows[1] - rows[0]} of {NJ} rows), two-launch route {w_at / 1e6:.1f} MB "
                 f"of whole streams: {100 * s_at / w_at:.1f} %")
    lines.append(f"  window route, pinned copy + 1 launch, host clock to a synchronise      {w_us:10.1f} us   (rounds {' '.join(f'{v:.0f}' for v in win)})")
    lines.append(f"    of which the pinned copy of the slices, same clock                   {cw_us:10.1f} us   {s_at / cw_us / 1e3:5.1f} GB/s")
    lines.append(f"    load_window_batch call (table upload + launch), device events        {kw_us:10.1f} us   {(read + out_bytes) / kw_us / 1e6:5.2f} TB/s of "
                 f"window values read ({read / 1e6:.1f} MB) + batch written")
    lines.append(f"  two-launch route, pinned copy + unpack + regrid, same host clock       {t_us:10.1f} us   (rounds {' '.join(f'{v:.0f}' for v in two)})")
    lines.append(f"    of which the pinned copy of the whole streams                        {ct_us:10.1f} us   {w_at / ct_us / 1e3:5.1f} GB/s")
    lines.append(f"    unpack + regrid calls (table uploads + 2 launches), device events    {kt_us:10.1f} us")
    lines.append(f"  ratio two-launch / window: end to end {t_us / w_us:.2f}, device part {kt_us / kw_us:.2f}; the outputs are equal bit for bit")
    return w_us, t_us


def loader_rates(files, dates, lines):
    root = tempfile.mkdtemp(prefix="p4c_grib_window_")
    try:
        g = np.random.default_rng(3)
        with open(os.path.join(root, "conf_PAAROME_1S40.grib"), "wb") as fh:
            fh.write(wc._grid_message(g, NJ, NI, 55.4, -12.0, 0.025, 16, 3, 6, 1, 0))
        for date, data in zip(dates, files):
            path = diskio.titan_grib_path(root, "AROME.grib", date)
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_bytes(data)
        meta = {"GRIDS": {"PAAROME_1S40": {"size": [NJ, NI], "extent": [55.4, 37.5, -12.0, 16.0]}},
                "WEATHER_PARAMS": {"aro_a": {"grib": "AROME.grib", "grid": "PAAROME_1S40", "long_name": "a", "param": "a", "type_level": "isobaricInhPa",
                                             "unit": "K", "name": "aro_a", "grib_keys": {"discipline": 0, "parameterCategory": 0,
                                                                                        "parameterNumber": 0, "typeOfFirstFixedSurface": 100}}}}
        conf = wc.titan_conf("grib")
        conf["grid"]["subdomain"] = list(SUB)
        conf["params"] = {"aro_a": {"levels": LEVELS, "kind": "input_output"}}
        conf["settings"]["standardize"] = False
        ds = datasets.NativeDataset.from_dict(datasets.TitanAccessor(root=root, metadata=meta), "titan", conf, 2, 3, 3)[0]
        n = len(ds)
        rates = {True: [], False: []}
        loaders = {use: datasets.DeviceLoader(ds, batch_size=B, shuffle=False, prefetch=2, threads=8, device=dev) for use in (True, False)}
        for use, loader in loaders.items():                                   # warm-up epoch: the files are parsed, the slots grown
            it = iter(loader)
            loader.routes.use_window = use
            for _ in it:
                pass
        for _ in range(5):
            for use, loader in loaders.items():
                torch.cuda.synchronize()
                t0, batches = time.perf_counter(), 0
                for _ in range(3):
                    for _ in loader:
                        batches += 1
                torch.cuda.synchronize()
                rates[use].append(batches / (time.perf_counter() - t0))
        counts = {use: dict(loader.routes.counts) for use, loader in loaders.items()}
        for loader in loaders.values():
            loader.close()
        lines.append(f"DeviceLoader over {len(dates)} dates = {n} samples of {T} steps, batches of {B}, files in the page cache, 8 threads, prefetch 2, "
                     f"5 alternating rounds of 3 epochs, no file parsed inside them:")
        for use, what in ((True, "window route   "), (False, "two-launch route")):
            lines.append(f"  {what} {statistics.median(rates[use]):8.2f} batches/s   (rounds {' '.join(f'{v:.2f}' for v in rates[use])}; groups by "
                         f"route {counts[use]})")
        return statistics.median(rates[True]), statistics.median(rates[False])
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "grib_window.txt"))
    args = ap.parse_args()
    lines = [f"Windowed decode of simple-packed GRIB2 fields on the target grid: tools/diagnostics/grib_window_time.py on {torch.cuda.get_device_name(0)}",
             "host clock around one call ending in a synchronise, 3 alternating rounds of 10 calls per route, median of the rounds' medians; "
             "launches with device events, median of 7 windows of 20 calls", ""]
    g = np.random.default_rng(0)
    dates = [dt.datetime(2023, 3, 1, h) for h in range(8)]
    files = messages(g, dates)
    w_us, t_us = device_routes(files, lines)
    lines.append("")
    r_w, r_t = loader_rates(files, dates, lines)
    lines.append("")
    faster = w_us <= t_us and r_w >= r_t
    lines.append(f"route of the loader for such a group: {'the window route' if faster else 'NOT DECIDED BY THESE FIGURES ALONE'} "
                 f"(GribRoutes.use_window): end to end {w_us:.0f} us against {t_us:.0f} us, {r_w:.2f} against {r_t:.2f} batches/s")
    lines.append("the device-event figures are taken around the Python call (descriptor table upload included), not from a kernel trace; a "
                 "'distinct message' is one (date, level): samples that overlap in a date share it and both routes copy it once")
    lines.append("not measured: files outside the page cache; an index that is not in the loader's cache (a shuffled order, more files than the "
                 "cache keeps: every batch then has its new files parsed by the reader threads before it can be laid out); widths other than 16 bits; the "
                 "eight-values-per-16-byte load (not built); what bounds the launch (its float64 arithmetic, the LDS read-out or its writes)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
