"""What profiles/datasets_native.txt holds: ops.pack_convert against the route without it, both starting from planes that lie in pinned
memory in the files' own dtype (where a reader's readinto puts them) -- without the kernel: numpy astype(float32) with the floor, the
scale and the flip into a second pinned buffer, the transfer, ops.pack_standardize; for untransformed f32 planes just the transfer and
ops.pack_standardize --, and datasets.DeviceLoader in batches per second on files in the page cache, reader threads and prefetch against
one thread and no prefetch.

    python tools/diagnostics/datasets_time.py [out.txt]
"""
import datetime as dt
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from py4cast_amd import datasets as D  # noqa: E402
from py4cast_amd import diskio, ops  # noqa: E402

dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def device_us(fn, calls=20, windows=7, warm=5):
    """median and spread over windows of `calls` back-to-back launches between two events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000 / calls)
    return statistics.median(out), min(out), max(out)


def wall_us(fn, n=9, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e6)
    return statistics.median(out), min(out), max(out)


def kernel_case(label, np_dtype, B, T, H, W, F, tr):
    rng = np.random.default_rng(0)
    if np.dtype(np_dtype).kind == "i":
        host = rng.integers(-50, 4000, (F, B, T, H, W)).astype(np_dtype)
    else:
        host = (rng.standard_normal((F, B, T, H, W)) * 5 + 280).astype(np_dtype)
    floor, div, mul, flip = tr
    mean, std = [0.7 + 0.01 * i for i in range(F)], [2.3 + 0.01 * i for i in range(F)]
    mean_d, std_d = torch.tensor(mean, device=dev), torch.tensor(std, device=dev)
    pinned = torch.from_numpy(host).pin_memory()
    raw = pinned.to(dev)
    feats = [(0, i, floor, div, mul, flip, mean[i], std[i], i) for i in range(F)]
    desc = ops.convert_features([raw], feats, B, T, H, W)
    k = device_us(lambda: ops.pack_convert_launch([raw], desc[0], desc[1], B, T, H, W))
    rows = B * T * H * W
    moved = rows * F * (host.dtype.itemsize + 4)
    say(f"{label}: {B}x{T}x{H}x{W}x{F} from {host.dtype}  (vec loads: {desc[1]})")
    say(f"  p4c_pack_convert            {k[0]:9.1f} us  ({k[1]:.1f} .. {k[2]:.1f})   {moved / k[0] / 1e6:6.2f} TB/s of {moved / 1e6:.1f} MB (source read + rows written)")
    plain_f32 = host.dtype == np.float32 and tr == (None, 1.0, 1.0, False)
    if plain_f32:
        ks = device_us(lambda: ops.pack_standardize(raw, mean_d, std_d))
        say(f"  p4c_pack_standardize, same planes {ks[0]:7.1f} us  ({ks[1]:.1f} .. {ks[2]:.1f})   (what the loader launches for untransformed f32 planes)")
    f32 = torch.empty(F, B, T, H, W, dtype=torch.float32).pin_memory()
    f32_np, typed_np = f32.numpy(), pinned.numpy()

    def old_route():   # without the kernel, from the pinned typed planes: host conversion and transform, fp32 over the link, pack_standardize
        if plain_f32:
            return ops.pack_standardize(pinned.to(dev, non_blocking=True), mean_d, std_d)
        v = typed_np.astype(np.float32)
        if floor is not None:
            v = np.where(v < 0, 0, v)
        if div != 1.0:
            v = v / np.float32(div) * np.float32(mul)
        if flip:
            v = v[..., ::-1, :]
        f32_np[...] = v
        return ops.pack_standardize(f32.to(dev, non_blocking=True), mean_d, std_d)

    def new_route():
        return ops.pack_convert([pinned.to(dev, non_blocking=True)], feats, B, T, H, W)

    o, n = wall_us(old_route), wall_us(new_route)
    what = "pinned copy + pack_standardize" if plain_f32 else "host astype/transform into pinned fp32 + copy + pack_standardize"
    say(f"  end to end, pinned typed planes -> packed batch: {what} {o[0]:9.0f} us ({o[1]:.0f} .. {o[2]:.0f});"
        f"  typed pinned copy + pack_convert {n[0]:9.0f} us ({n[1]:.0f} .. {n[2]:.0f});  ratio {o[0] / n[0]:.2f}")


def loader_case(label, ds, batch_size, step_ms=5.0, batches=12):
    for threads, prefetch in ((1, 0), (8, 2)):
        with D.DeviceLoader(ds, batch_size=batch_size, device=dev, threads=threads, prefetch=prefetch) as loader:
            for _, b in zip(range(2), loader):        # page cache, pinned buffers, kernels' first launches
                pass
            torch.cuda.synchronize()
            loader.waited_s = 0.0
            t = time.perf_counter()
            n = 0
            for _, b in zip(range(batches), loader):
                n += 1
            torch.cuda.synchronize()
            free = (time.perf_counter() - t) / n
            loader.waited_s = 0.0
            t = time.perf_counter()
            n = 0
            for _, b in zip(range(batches), loader):
                time.sleep(step_ms / 1e3)                # the stand-in step
                n += 1
            torch.cuda.synchronize()
            busy = (time.perf_counter() - t) / n
            say(f"  {label} threads={threads} prefetch={prefetch}: {1 / free:7.1f} batches/s with nothing between batches; with a {step_ms:.0f} ms stand-in "
                f"step {busy * 1e3:6.1f} ms per batch, of which the consumer waited {loader.waited_s / n * 1e3:6.2f} ms for reads")


def rainfall_dataset(root):
    t0s = [dt.datetime(2024, 1, 1) + k * dt.timedelta(seconds=10800) for k in range(16)]
    rng = np.random.default_rng(1)
    for t0 in t0s:
        for d in range(-1, 4):
            date = t0 + d * dt.timedelta(seconds=300)
            path = os.path.join(root, "Hexagone", str(date.year), date.strftime("%Y%m%d%H%M") + ".npz")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.savez(path, rng.integers(-1, 3000, (1536, 1536)).astype(np.int16))
    conf = {"grid": {"name": "rainfallgrid", "border_size": 0},
            "params": {"precip": {"levels": [0], "kind": "input_output"}},
            "periods": {p: dict(start=20240101, end=20240102, obs_step=300, obs_step_btw_t0=10800) for p in ("train", "valid", "test")},
            "settings": {"standardize": True, "file_format": "npz"}}
    acc = D.RainfallAccessor(root=root)
    _, valid, _ = D.NativeDataset.from_dict(acc, "rainfall", conf, 2, 1, 3)
    diskio.save_stats({"precip": {"mean": 0.7, "std": 2.3}}, os.path.join(valid.cache_dir, "parameters_stats.pt"))
    return valid


def titan_dataset(root, H=512, W=640):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests"))
    import grib2_reference as gr

    levels = [1000, 950, 925, 900, 850, 800, 750, 700, 600, 500, 400, 300, 250, 200, 150, 100, 50, 20, 10, 5, 1]   # 21 planes
    meta = {"GRIDS": {"PAAROME_1S100": {"size": [H, W]}},
            "WEATHER_PARAMS": {"aro_t": {"grib": "x.grib", "grid": "PAAROME_1S40", "long_name": "t", "param": "t", "type_level": "isobaricInhPa", "unit": "K"}}}
    rng = np.random.default_rng(2)
    height = (rng.random(H * W) * 900).astype(np.float32)
    with open(os.path.join(root, "conf_PAAROME_1S100.grib"), "wb") as f:
        f.write(gr.message(0, gr.section1(dt.datetime(2020, 1, 1)), gr.section3(False, ni=W, nj=H), gr.section4(3, 6, 1, None), height, 1, 16))
    acc = D.TitanAccessor(root=root, metadata=meta)
    conf = {"grid": {"name": "PAAROME_1S100", "border_size": 0, "subdomain": [0, H, 0, W]},
            "params": {"aro_t": {"levels": levels, "kind": "input_output"}},
            "periods": {p: dict(start=20230301, end=20230301, obs_step=3600, obs_step_btw_t0=3600) for p in ("train", "valid", "test")},
            "settings": {"standardize": True, "file_format": "npy"}}
    sub = os.path.join(root, "subdatasets", f"titan_PAAROME_1S100_0-{H}-0-{W}")
    for hour in range(24):
        date = dt.datetime(2023, 3, 1, hour)
        os.makedirs(os.path.join(sub, "data", date.strftime("%Y-%m-%d_%Hh%M")), exist_ok=True)
        for lv in levels:
            np.save(os.path.join(sub, "data", date.strftime("%Y-%m-%d_%Hh%M"), f"aro_t_{lv}hpa.npy"),
                    (rng.standard_normal((H, W)) * 5 + 250).astype(np.float32))
    diskio.save_stats({f"aro_t_{lv}hpa": {"mean": 250.0, "std": 5.0} for lv in levels}, os.path.join(sub, "parameters_stats.pt"))
    train, _, _ = D.NativeDataset.from_dict(acc, "titan", conf, 1, 3, 3)
    return train


if __name__ == "__main__":
    say(f"{torch.cuda.get_device_name(0)}; device times: median (min .. max) of 7 windows of 20 launches between two events; "
        f"end-to-end times: median (min .. max) of 9 synchronised calls")
    kernel_case("rainfall", np.int16, 1, 5, 1536, 1536, 1, (0.0, 100.0, 12.0, True))
    kernel_case("titan f32", np.float32, 2, 4, 512, 640, 21, (None, 1.0, 1.0, False))
    kernel_case("titan f64", np.float64, 2, 4, 512, 640, 21, (None, 1.0, 1.0, False))
    say()
    say("DeviceLoader, files in the PAGE CACHE (written just before, read twice before timing): no disk is measured here")
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "rain"))
        os.makedirs(os.path.join(tmp, "titan"))
        loader_case("rainfall 1x5x1536x1536x1 int16 npz (stored)", rainfall_dataset(os.path.join(tmp, "rain")), 1)
        loader_case("titan-npy 2x4x512x640x21 f32", titan_dataset(os.path.join(tmp, "titan")), 2)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")
