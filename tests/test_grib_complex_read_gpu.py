"""
The GRIB reader on the GPU with complex-packed messages (templates 5.2 / 5.3): ``diskio.GribPlaneReader`` on files that mix them with
simple packing against its own host path and against the integers that went into the files, the ``check`` of a malformed file, and
``load_titan_grib_batch`` on complex-packed files against the same call on 5.0 files of the same integers.  Bit for bit.
"""
import datetime as dt
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_complex_cases as cc  # noqa: E402
import grib_unpack_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
DATES = [dt.datetime(2023, 5, 1, 0) + dt.timedelta(hours=h) for h in range(3)]


class Stats:
    def __init__(self, mean, std):
        self.d = {"mean": mean, "std": std}

    def to_list(self, stat, names, dtype=torch.float32):
        return self.d[stat].type(dtype)


@pytest.mark.parametrize("south_to_north", [False, True])
def test_the_device_reader_on_files_that_mix_the_templates(south_to_north, gpu_device, tmp_path):
    """23 x 39 points, no multiple of 4: the planes lie at a pitch, each decode writes its own planes of the one output"""
    from py4cast_amd import ops
    from py4cast_amd.diskio import GribPlaneReader

    paths, fids, wants = [], None, []
    for t in range(2):
        data, fids, planes = cc.mixed_file(south_to_north, seed=6 + t)
        paths.append(tmp_path / f"mixed{t}.grib")
        paths[-1].write_bytes(data)
        wants.append(planes)
    selections = [[[(path, fid) for path in paths]] for fid in fids]                              # F = 4, B = 1, T = 2
    host, lat_h, lon_h = GribPlaneReader(device=None).read(selections)
    reader = GribPlaneReader(device=gpu_device)
    for _ in range(2):
        dev, lat, lon = reader.read(selections)
        torch.cuda.synchronize()
        assert tuple(dev.shape) == (4, 1, 2, 23, 39) and not dev.is_contiguous() and ops.planes_dense(dev) and dev.stride(2) == 900
        got = dev.cpu().numpy()
        assert cases.same_bits(got, host.numpy())
        for f in range(4):
            for t in range(2):
                assert cases.same_bits(got[f, 0, t], wants[t][f]), (f, t)
        assert np.array_equal(lat, lat_h) and np.array_equal(lon, lon_h) and lat[0] > lat[-1]
        assert reader.last_status.tolist() == [0] * 6
    assert np.isnan(got[2]).any() and not np.isnan(got[[0, 1, 3]]).any()
    # complex-packed messages alone, and simple ones alone: the latter leave no status behind
    only = GribPlaneReader(device=gpu_device, check=False)
    assert cases.same_bits(only.read(selections[1:])[0].cpu().numpy(), host.numpy()[1:]) and only.last_status.tolist() == [0] * 6
    assert cases.same_bits(only.read(selections[:1])[0].cpu().numpy(), host.numpy()[:1]) and only.last_status is None


@pytest.mark.parametrize("kind", ["lengths", "width", "stream"])
def test_the_check_names_a_malformed_file(kind, gpu_device, tmp_path):
    from py4cast_amd import grib2
    from py4cast_amd.diskio import GribPlaneReader

    g = np.random.default_rng(21)
    ni, nj = 9, 5
    f = cc.smooth_field(g, ni * nj)
    good, bad = tmp_path / "good.grib", tmp_path / "bad.grib"
    good.write_bytes(cc.message(ni, nj, f, 1, [0, 20], 1.5, -2, 1))
    msg, bit, _ = cc.malformed(kind)
    bad.write_bytes(msg)
    fid = {"discipline": 0, "parameterCategory": 0, "parameterNumber": 0}
    selections = [[[(good, fid), (bad, fid), (good, fid)]]]
    words = {"lengths": "group lengths do not sum", "width": "group width above 32", "stream": "more bits than section 7 holds"}[kind]
    with pytest.raises(grib2.GribError, match=re.escape(str(bad)) + ".*" + words):
        GribPlaneReader(device=gpu_device).read(selections)
    with pytest.raises(grib2.GribError, match=re.escape(str(bad))):
        GribPlaneReader(device=None).read(selections)
    reader = GribPlaneReader(device=gpu_device, check=False)
    planes, _, _ = reader.read(selections)
    st = reader.last_status.tolist()
    assert st[0] == 0 and st[2] == 0 and st[1] & bit
    got = planes.cpu().numpy()[0, 0]
    want = cc.expected_plane(f, ni, nj, 1.5, -2, 1)
    assert np.isnan(got[1]).all() and cases.same_bits(got[0], want) and cases.same_bits(got[2], want)


def _write_dataset(root, packing, nj, ni):
    """<root>/grib/<date>/{a,b}.grib with the same integers either way: packing "simple" writes 5.0 at 16 bits, "complex" 5.2 and 5.3"""
    from py4cast_amd.diskio import titan_grib_path

    g, gb = np.random.default_rng(30), np.random.default_rng(31)     # the fields are the same either way; the groups draw from gb
    n = ni * nj
    for date in DATES:
        for fname, south_to_north, numbers in (("a.grib", True, ((0, 0), (2, 2))), ("b.grib", False, ((1, 1), (3, 1)))):
            out = []
            for i, (category, number) in enumerate(numbers):
                f = cc.smooth_field(g, n, amplitude=9000, offset=20000, noise=30)              # 0 <= f < 2^16
                R, E, D = float(np.float32(g.normal() * 50)), -4, (2, 0)[i]
                if packing == "simple":
                    out.append(cases.message(ni, nj, f.astype(np.uint64), 16, R, E, D, south_to_north=south_to_north, category=category,
                                             number=number))
                else:
                    order = (2, 0)[i] if fname == "a.grib" else (1, 2)[i]
                    out.append(cc.message(ni, nj, f, order, cc.random_bounds(gb, n), R, E, D, south_to_north=south_to_north,
                                          category=category, number=number, nbytes=3))
            path = titan_grib_path(root, fname, date)
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_bytes(b"".join(out))


@pytest.mark.parametrize("resize,grid", [(False, (24, 40)), (True, (23, 39))])
def test_the_grib_batch_of_complex_packed_files_equals_that_of_simple_packed_ones(resize, grid, gpu_device, tmp_path):
    from py4cast_amd import regrid
    from py4cast_amd.diskio import load_titan_grib_batch

    fid = lambda c, p: {"discipline": 0, "parameterCategory": c, "parameterNumber": p}   # noqa: E731
    params = [("t", "a.grib", fid(0, 0), "A"), ("p", "b.grib", fid(3, 1), "B"), ("u", "a.grib", fid(2, 2), "A"), ("c", "b.grib", fid(1, 1), "B")]
    full = (36, 52) if resize else grid
    plans = {name: regrid.RegridPlan(grid, full, subdomain=(2, full[0] - 2, 4, full[1] - 4)) for name in ("A", "B")}
    dates = [[DATES[0], DATES[1]], [DATES[1], DATES[2]]]
    g = torch.Generator().manual_seed(1)
    stats = Stats(torch.randn(4, generator=g) * 5, torch.rand(4, generator=g) + 0.5)
    batches = {}
    for packing in ("simple", "complex"):
        root = tmp_path / packing
        _write_dataset(root, packing, grid[0], grid[1])
        batches[packing] = load_titan_grib_batch(root, params, dates, stats, 1, None, plans, device=gpu_device)
    got, want = batches["complex"], batches["simple"]
    H, W = plans["A"].out_shape
    assert got.inputs.tensor.shape == (2, 1, H, W, 4) and got.inputs.feature_names == [p[0] for p in params]
    for a, b in ((got.inputs.tensor, want.inputs.tensor), (got.outputs.tensor, want.outputs.tensor)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(torch.isfinite(a).all())
    assert float(got.inputs.tensor.std()) > 0.1
