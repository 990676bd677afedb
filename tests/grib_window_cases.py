"""
What the tests of the windowed GRIB decode share (test infrastructure, never product code; not collected): fields around random
integers built with tests/grib_unpack_cases.py, the expected window from ``grib2.decode`` (flip, crop, two float32 steps), the slices
of a call in one byte buffer with a chosen filler between and after them, and a tiny Titan tree in GRIB.
"""
import datetime as dt
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_unpack_cases as cases  # noqa: E402

NBITS = (0, 1, 7, 12, 16, 24, 31, 32)
DS = (-2, 0, 3)
NJ, NI = 29, 37


def expected_window(msg, window, mean=0.0, std=1.0):
    """``grib2.decode`` of the message, rounded to float32, north-first (a south-to-north file flipped), cropped to ``window`` =
    (r0, r1, c0, c1), then (v - mean) / std in float32 steps"""
    from py4cast_amd import grib2

    plane = cases.expected_plane(msg, flip=grib2.field_of(msg).south_to_north)
    r0, r1, c0, c1 = window
    f4 = np.float32
    with np.errstate(all="ignore"):
        return ((plane[r0:r1, c0:c1] - f4(mean)) / f4(std)).astype(f4)


def fid(f):
    """the numeric keys of feature f's messages in the files of ``write_files``"""
    return {"discipline": 0, "parameterCategory": f // 8, "parameterNumber": f % 8}


def spec_of(f, g):
    """feature f of a mixed call -> (nbits, R, E, D)"""
    return NBITS[f % 8], float(np.float32(g.normal() * 40)), (-5, -3, 0, 2)[f % 4], DS[f % 3]


def messages(g, B, T, specs, nj=NJ, ni=NI, scan=None):
    """msgs[f][b][t]: one message per (feature, sample, step) around random integers; specs[f] = (nbits, R, E, D); scan(f, b, t) ->
    south_to_north (default: alternating with b + t)"""
    scan = scan or (lambda f, b, t: bool((b + t) % 2))
    return [[[cases.random_message(g, ni, nj, nbits, R, E, D, south_to_north=scan(f, b, t), category=f // 8, number=f % 8)
              for t in range(T)] for b in range(B)] for f, (nbits, R, E, D) in enumerate(specs)]


def write_files(root, msgs):
    """one file per (b, t) that holds the messages of all features -> selections[f][b][t] = (path, fid) for ``GribPlaneReader.read``"""
    F, B, T = len(msgs), len(msgs[0]), len(msgs[0][0])
    for b in range(B):
        for t in range(T):
            with open(os.path.join(root, f"b{b}t{t}.grib"), "wb") as fh:
                fh.write(b"".join(msgs[f][b][t] for f in range(F)))
    return [[[(os.path.join(root, f"b{b}t{t}.grib"), fid(f)) for t in range(T)] for b in range(B)] for f in range(F)]


def slices_buffer(fields, rows, fill, lead=4, gap=8, tail=16):
    """The slices of fields[f][b][t] over the north-first plane rows ``rows`` in one byte buffer: ``lead`` filler bytes, every slice
    at a multiple of 4 with at least ``gap`` filler bytes after it (the bytes up to the next multiple of 4 included), ``tail`` more
    at the end -> (uint8 array, places[f][b][t] = (slice_off, slice_len, bit0))"""
    from py4cast_amd import grib2

    chunks, at, places = [bytes([fill]) * lead], lead, []
    for per_f in fields:
        places.append([])
        for per_b in per_f:
            places[-1].append([])
            for f in per_b:
                start, end, bit0 = grib2.window_slice(f, *rows)
                data = bytes(f.stream[start:end])
                pad = -len(data) % 4 + gap
                places[-1][-1].append((at, len(data), bit0))
                chunks.append(data + bytes([fill]) * pad)
                at += len(data) + pad
    chunks.append(bytes([fill]) * tail)
    return np.frombuffer(b"".join(chunks), dtype=np.uint8).copy(), places


class Stats:
    """``Stats.to_list`` over a dict name -> (mean, std)"""

    def __init__(self, table):
        self.table = dict(table)

    def to_list(self, stat, names, dtype=None):
        import torch

        return torch.tensor([self.table[n][0 if stat == "mean" else 1] for n in names], dtype=dtype or torch.float32)


# ------------------------------------------------------------------------------------------------ a tiny Titan tree in GRIB
# target grid PAAROME_1S40 on 29 x 37 points; "aro_a" (two levels) lies on it, "arp_b" on a PA_01D-like grid of 16 x 20 coarser points
GRID_STEP, ARP_STEP = 0.025, 0.05
LAT_N, LON_W = 50.0, 2.0
ARP_NJ, ARP_NI = 18, 22
TITAN_DATES = [dt.datetime(2023, 3, 1, h) for h in range(3)]
SUBDOMAIN = (4, 23, 6, 29)


def titan_metadata(keys=True):
    lat_s, lon_e = LAT_N - (NJ - 1) * GRID_STEP, LON_W + (NI - 1) * GRID_STEP
    aro = {"grib": "AROME.grib", "grid": "PAAROME_1S40", "long_name": "field a", "param": "a", "type_level": "isobaricInhPa",
           "unit": "K", "name": "aro_a"}
    arp = {"grib": "ARPEGE.grib", "grid": "PA_01D", "long_name": "field b", "param": "b", "type_level": "heightAboveGround", "unit": "K",
           "name": "arp_b"}
    if keys:
        aro["grib_keys"] = {"discipline": 0, "parameterCategory": 0, "parameterNumber": 0, "typeOfFirstFixedSurface": 100}   # no level
        arp["grib_keys"] = {"discipline": 0, "parameterCategory": 1, "parameterNumber": 1, "level": 2}
    return {"GRIDS": {"PAAROME_1S40": {"size": [NJ, NI], "extent": [LAT_N, lat_s, LON_W, lon_e]}},
            "WEATHER_PARAMS": {"aro_a": aro, "arp_b": arp}}


def titan_conf(file_format="grib", dates=("20230301", "20230301")):
    period = {"start": int(dates[0]), "end": int(dates[1]), "obs_step": 3600, "obs_step_btw_t0": 3600}
    return {"grid": {"name": "PAAROME_1S40", "border_size": 2, "subdomain": list(SUBDOMAIN), "proj_name": "PlateCarree", "projection_kwargs": {}},
            "params": {"aro_a": {"levels": [850, 500], "kind": "input_output"}, "arp_b": {"levels": [2], "kind": "input"}},
            "periods": {"train": dict(period), "valid": dict(period), "test": dict(period)},
            "settings": {"standardize": True, "file_format": file_format}}


def _grid_message(g, nj, ni, lat_n, lon_w, step, nbits, category, number, surface, level, south_to_north=False, present=None, D=2):
    """a message on an nj x ni grid whose northern row is lat_n and western column lon_w"""
    import struct

    import grib2_reference as ref

    micro = lambda x: int(round(x * 1e6))  # noqa: E731
    la_n, la_s = micro(lat_n), micro(lat_n - (nj - 1) * step)
    la1, la2 = (la_s, la_n) if south_to_north else (la_n, la_s)
    body = (struct.pack(">BIBBH", 0, ni * nj, 0, 0, 0) + bytes([6]) + b"\xff" * 15 + struct.pack(">IIII", ni, nj, 0, 0xFFFFFFFF)
            + ref.sm(la1, 4) + ref.sm(micro(lon_w), 4) + bytes([0x30]) + ref.sm(la2, 4) + ref.sm(micro(lon_w + (ni - 1) * step), 4)
            + struct.pack(">IIB", micro(step), micro(step), 0x40 if south_to_north else 0))
    s3 = struct.pack(">IB", 5 + len(body), 3) + body
    n = ni * nj if present is None else int(np.count_nonzero(present))
    X = g.integers(0, 2 ** nbits, size=n, dtype=np.uint64)
    stream = X.astype(">u2").tobytes() if nbits == 16 else cases.stream_of(X, nbits)      # whole octets: no bit matrix needed
    s6 = struct.pack(">IBB", 6, 6, 255) if present is None else \
        struct.pack(">IBB", 6 + (ni * nj + 7) // 8, 6, 0) + np.packbits(np.asarray(present, dtype=np.uint8)).tobytes()
    parts = [ref.section1(dt.datetime(2020, 1, 1)), s3, ref.section4(category, number, surface, (0, level)),
             ref.section5(n, float(np.float32(250 + 10 * category)), -6, D, nbits), s6, struct.pack(">IB", 5 + len(stream), 7) + stream, b"7777"]
    return b"GRIB\x00\x00" + bytes([0, 2]) + struct.pack(">Q", 16 + sum(len(p) for p in parts)) + b"".join(parts)


def write_titan_tree(root, dates=TITAN_DATES, bitmap=False, skip=()):
    """<root>/conf_PAAROME_1S40.grib and, per date, <root>/grib/<date>/{AROME,ARPEGE}.grib: AROME.grib (scans south to north) holds
    aro_a at 850 and 500 hPa in 16 and 12 bits on the target grid (with ``bitmap``: a bitmap on the 500 hPa field, every point but
    the first present), ARPEGE.grib (north to south) arp_b at 2 m on the coarser grid around it.  skip: (date, file name) not written."""
    from py4cast_amd.diskio import titan_grib_path

    g = np.random.default_rng(5)
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "conf_PAAROME_1S40.grib"), "wb") as fh:
        fh.write(_grid_message(g, NJ, NI, LAT_N, LON_W, GRID_STEP, 16, 3, 6, 1, 0))
    for date in dates:
        present = None
        if bitmap:
            present = np.ones(NJ * NI, dtype=bool)
            present[0] = False
        files = {"AROME.grib": _grid_message(g, NJ, NI, LAT_N, LON_W, GRID_STEP, 16, 0, 0, 100, 850, south_to_north=True)
                 + _grid_message(g, NJ, NI, LAT_N, LON_W, GRID_STEP, 12, 0, 0, 100, 500, south_to_north=True, present=present),
                 "ARPEGE.grib": _grid_message(g, ARP_NJ, ARP_NI, LAT_N + 2 * ARP_STEP, LON_W - 2 * ARP_STEP, ARP_STEP, 16, 1, 1, 103, 2)}
        for name, data in files.items():
            if (date, name) in skip:
                continue
            path = titan_grib_path(root, name, date)
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_bytes(data)


def titan_datasets(root, file_format="grib", keys=True, steps=(1, 1, 1), metadata=None):
    from py4cast_amd import datasets as D

    acc = D.TitanAccessor(root=root, metadata=metadata or titan_metadata(keys))
    return D.NativeDataset.from_dict(acc, "titan", titan_conf(file_format), *steps)


def titan_stats(ds):
    """statistics files for the tiny tree: other values per feature"""
    from py4cast_amd import diskio

    names = [ds.accessor.parameter_namer(p) for p in ds.params]
    os.makedirs(ds.cache_dir, exist_ok=True)
    table = {n: {"mean": 240.0 + 7 * i, "std": 3.0 + i, "min": 0.0, "max": 400.0} for i, n in enumerate(names)}
    diskio.save_stats(table, os.path.join(ds.cache_dir, "parameters_stats.pt"))
    diskio.save_stats({n: {"mean": 0.0, "std": 1.0} for n in names}, os.path.join(ds.cache_dir, "diff_stats.pt"))
