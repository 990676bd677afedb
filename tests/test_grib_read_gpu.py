"""
The GRIB reader on the GPU: ``diskio.GribPlaneReader`` against its own host path, ``load_titan_grib_batch`` against
``datapipe.load_native_batch`` fed with host-decoded planes, and files written by ``ForecastGribWriter`` read back.  Everything is
compared bit for bit: the device decode is the host decode (tests/test_grib_unpack_gpu.py), and what follows it is the same launch.
"""
import datetime as dt
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib2_reference as ref  # noqa: E402
import grib_unpack_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
NJ, NI = ref.NJ, ref.NI                                    # 24 x 40
#         name  (category, number)  nbits   D   bitmap
PARAMS = [("t", (0, 0), 16, 2, False), ("u", (2, 2), 12, 0, True), ("c", (1, 1), 0, -1, False), ("p", (3, 1), 16, -1, True)]
DATES = [dt.datetime(2023, 5, 1, 0) + dt.timedelta(hours=h) for h in range(3)]


class Stats:
    def __init__(self, mean, std):
        self.d = {"mean": mean, "std": std}

    def to_list(self, stat, names, dtype=torch.float32):
        return self.d[stat].type(dtype)


def _fid(name):
    category, number = next(p[1] for p in PARAMS if p[0] == name)
    return {"discipline": 0, "parameterCategory": category, "parameterNumber": number}


def _write_dataset(root, bitmaps=True, nj=NJ, ni=NI):
    """<root>/grib/<date>/{a,b}.grib: a.grib scans south to north and holds t and u, b.grib north to south with c and p; other values
    at every date"""
    from py4cast_amd.diskio import titan_grib_path

    g = np.random.default_rng(30)
    for date in DATES:
        for fname, south_to_north, names in (("a.grib", True, ("t", "u")), ("b.grib", False, ("c", "p"))):
            out = []
            for name, (category, number), nbits, D, bitmap in PARAMS:
                if name in names:
                    present = (g.random(nj * ni) < 0.8) if (bitmap and bitmaps) else None
                    out.append(cases.random_message(g, ni, nj, nbits, float(np.float32(g.normal() * 50)), -4, D, present=present,
                                                    south_to_north=south_to_north, category=category, number=number))
            path = titan_grib_path(root, fname, date)
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_bytes(b"".join(out))
    return {"t": "a.grib", "u": "a.grib", "c": "b.grib", "p": "b.grib"}


def test_the_device_reader_equals_the_host_reader(gpu_device, tmp_path):
    from py4cast_amd.diskio import GribPlaneReader, titan_grib_path

    where = _write_dataset(tmp_path)
    # F = 4, B = 2, T = 2 over two files per date; the samples overlap in one date: its messages are copied once
    selections = [[[(titan_grib_path(tmp_path, where[n], DATES[b + t]), _fid(n)) for t in range(2)] for b in range(2)] for n, *_ in PARAMS]
    host, lat_h, lon_h = GribPlaneReader(device=None).read(selections)
    reader = GribPlaneReader(device=gpu_device)
    for _ in range(2):                                       # the second call reuses the pinned buffer and the parsed files
        dev, lat, lon = reader.read(selections)
        torch.cuda.synchronize()
        assert dev.device == gpu_device and dev.dtype == torch.float32 and tuple(dev.shape) == (4, 2, 2, NJ, NI) and dev.is_contiguous()
        assert cases.same_bits(dev.cpu().numpy(), host.numpy())
        assert np.array_equal(lat, lat_h) and np.array_equal(lon, lon_h) and lat[0] > lat[-1]
    assert reader.parsed == 6 and reader.host.is_pinned()
    nan = torch.isnan(host)
    assert nan[1].any() and nan[3].any() and not nan[0].any() and not nan[2].any()              # the bitmaps are where they belong
    assert (host[2].std(dim=(-1, -2)) == 0).all() and host[0].std() > 1                          # the 0-bit field is constant
    # a grid of 23 x 39 points, no multiple of 4: every plane is dense and 16-byte aligned, at a pitch, and nothing was copied
    g = np.random.default_rng(2)
    odd = tmp_path / "odd.grib"
    odd.write_bytes(cases.random_message(g, 39, 23, 10, 3.0, -2, 1) + cases.random_message(g, 39, 23, 16, 3.0, -2, 1, category=2, number=2))
    sel = [[[(odd, _fid("t"))]], [[(odd, _fid("u"))]]]
    dev, _, _ = reader.read(sel)
    from py4cast_amd import ops

    assert not dev.is_contiguous() and ops.planes_dense(dev) and dev.stride(0) == 900 and all(dev[i].data_ptr() % 16 == 0 for i in range(2))
    assert tuple(dev.shape) == (2, 1, 1, 23, 39) and cases.same_bits(dev.cpu().numpy(), GribPlaneReader(device=None).read(sel)[0].numpy())


@pytest.mark.parametrize("resize,grid", [(False, (NJ, NI)), (True, (NJ, NI)), (False, (23, 39)), (True, (23, 39))])
def test_the_grib_batch_equals_the_native_batch_of_host_decoded_planes(resize, grid, gpu_device, tmp_path):
    """on 23 x 39 points, no multiple of 4, the reader's planes lie at a pitch and go into the regrid launch as they are"""
    from py4cast_amd import datapipe, regrid
    from py4cast_amd.diskio import GribPlaneReader, load_titan_grib_batch, titan_grib_path

    where = _write_dataset(tmp_path, bitmaps=False, nj=grid[0], ni=grid[1])          # a NaN would spread through the resize: the equality below needs numbers
    full = (36, 52) if resize else grid
    plans = {name: regrid.RegridPlan(grid, full, subdomain=(2, full[0] - 2, 4, full[1] - 4)) for name in ("A", "B")}
    params = [("t", where["t"], _fid("t"), "A"), ("p", where["p"], _fid("p"), "B"), ("u", where["u"], _fid("u"), "A"), ("c", where["c"], _fid("c"), "B")]
    names = [p[0] for p in params]
    dates = [[DATES[0], DATES[1]], [DATES[1], DATES[2]]]
    g = torch.Generator().manual_seed(1)
    stats = Stats(torch.randn(4, generator=g) * 5, torch.rand(4, generator=g) + 0.5)
    batch = load_titan_grib_batch(tmp_path, params, dates, stats, 1, None, plans, device=gpu_device)
    groups = []
    for name in ("A", "B"):
        mine = [p for p in params if p[3] == name]
        sel = [[[(titan_grib_path(tmp_path, fname, d), fid) for d in sample] for sample in dates] for _, fname, fid, _ in mine]
        groups.append((GribPlaneReader(device=None).read(sel)[0].to(gpu_device), [p[0] for p in mine], plans[name]))
    want = datapipe.load_native_batch(groups, names, None, stats, 1)
    H, W = plans["A"].out_shape
    assert batch.inputs.tensor.shape == (2, 1, H, W, 4) and batch.outputs.tensor.shape == (2, 1, H, W, 4)
    assert batch.inputs.feature_names == batch.outputs.feature_names == names and batch.forcing is None
    for got, ref_t in ((batch.inputs.tensor, want.inputs.tensor), (batch.outputs.tensor, want.outputs.tensor)):
        assert torch.equal(got.view(torch.int32), ref_t.view(torch.int32)) and bool(torch.isfinite(got).all())
    assert float(batch.inputs.tensor.std()) > 0.1


@pytest.mark.parametrize("south_to_north", [True, False])
def test_files_of_the_forecast_writer_read_back(south_to_north, gpu_device, tmp_path):
    """ForecastGribWriter writes an 18 x 28 forecast into the 24 x 40 template grid: a bitmap.  Read back on the device, the window
    equals ``grib2.decode`` of the same files and everything outside it is NaN."""
    from py4cast_amd import grib2
    from py4cast_amd.diskio import GribPlaneReader
    from py4cast_amd.namedtensor import NamedTensor
    from py4cast_amd.outputs import ForecastGribWriter, GribSample, OutputSavingSettings, grib_fid

    names = ["aro_t2m_2m", "aro_u10_10m", "aro_prmsl_0hpa", "aro_r2_2m"]
    pred = torch.randn(1, 2, ref.H, ref.W, len(names), generator=torch.Generator().manual_seed(9))
    std, mean = torch.tensor([6.0, 4.0, 900.0, 20.0]), torch.tensor([283.0, -1.0, 101300.0, 60.0])
    lat, lon = ref.forecast_grid()
    (tmp_path / "gribs").mkdir()
    (tmp_path / "template.grib").write_bytes(ref.template_file(south_to_north=south_to_north))
    io = tmp_path / "io.json"
    io.write_text(json.dumps({"template_grib": "../template.grib", "path_to_runtime": "{}", "dir_grib": str(tmp_path / "gribs"),
                              "dir_gif": str(tmp_path / "gifs"), "grib_fmt": "mb{}_ech_{}.grib", "grib_identifiers": ["member", "leadtime"]}))
    writer = ForecastGribWriter(OutputSavingSettings.from_json(io), gpu_device, lat, lon)
    start = dt.datetime(2023, 1, 1, 6)
    deltas = [dt.timedelta(hours=i - 1) for i in range(4)]
    sample = types.SimpleNamespace(timestamps=types.SimpleNamespace(datetime=start, timedeltas=deltas), member=0,
                                   output_timestamps=types.SimpleNamespace(datetime=start, timedeltas=deltas[2:]))
    preds = NamedTensor(pred.to(gpu_device), ["batch", "timestep", "lat", "lon", "features"], list(names))
    writer.submit(preds, std.to(gpu_device), mean.to(gpu_device), [GribSample.from_sample(sample, "2023010106")])
    writer.drain()
    files = sorted(writer.written)
    assert len(files) == 2
    fids = [grib_fid(n, 3600)[0] for n in names]
    selections = [[[(path, fid) for path in files]] for fid in fids]                              # F = 4, B = 1, T = 2
    planes, rlat, rlon = GribPlaneReader(device=gpu_device).read(selections)
    got = planes.cpu().numpy()
    inside = np.zeros((ref.NJ, ref.NI), dtype=bool)
    inside[ref.ROW0:ref.ROW0 + ref.H, ref.COL0:ref.COL0 + ref.W] = True                           # in south-to-north rows
    inside = inside[::-1]                                                                         # plane row 0 is the northernmost
    for f, fid in enumerate(fids):
        for t, path in enumerate(files):
            m = grib2.GribFile(path).find(fid)
            assert m.keys["bitMapIndicator"] == 0 and bool(m.keys["scanningMode"] & 0x40) == south_to_north
            want = cases.expected_plane(m, flip=south_to_north)
            assert np.array_equal(np.isnan(want), ~inside)
            assert cases.same_bits(got[f, 0, t], want), (names[f], t)
    assert np.isnan(got[:, :, :, ~inside]).all() and np.isfinite(got[:, :, :, inside]).all()
    # and the values are the prediction's, to the packing step: row 0 of the forecast grid is the southern one
    v = (pred[0, :, :, :, 0] * std[0] + mean[0]).numpy()[:, ::-1]
    assert np.abs(got[0, 0][:, inside].reshape(2, ref.H, ref.W) - v).max() < 0.01
    assert rlat[0] > rlat[-1] and np.allclose(rlat[::-1][ref.ROW0:ref.ROW0 + ref.H], lat[:, 0], atol=1e-6)
