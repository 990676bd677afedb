"""
``DeviceLoader`` over a Titan GRIB dataset and ``diskio.convert_titan_grib_to_npy`` on the GPU.  The tree (tests/grib_window_cases.py):
two GRIB files per date, five dates, ``aro_a`` at two levels on the target grid (the window route) and ``arp_b`` on a coarser grid (the
regrid route).  Every batch is compared with ``torch.equal`` against ``diskio.load_titan_grib_batch`` -- whole streams, unpack, regrid
-- on the same dates; which route a group took is read from the loader's counters.
"""
import datetime as dt
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_window_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu
DATES = [dt.datetime(2023, 3, 1, h) for h in range(5)]
STEPS = (2, 1, 1)                                   # two input steps, one prediction step: three samples over five dates


def _dataset(root, file_format="grib", bitmap=False):
    wc.write_titan_tree(root, dates=DATES, bitmap=bitmap)
    ds = wc.titan_datasets(root, file_format, steps=STEPS)[0]
    wc.titan_stats(ds)
    return ds


def _expected(ds, samples, device, standardize=True):
    """the batch of ``samples`` from ``load_titan_grib_batch`` (one ``GribPlaneReader`` call per native grid, ``load_native_batch``)
    and ``ops.build_forcing``"""
    from py4cast_amd import forcings, grib2, ops
    from py4cast_amd.diskio import load_titan_grib_batch, titan_grib_path

    acc, root = ds.accessor, ds.accessor.root
    plans = {}
    for p in ds.params:
        m, f = grib2.GribFile(titan_grib_path(root, p.grib_name, DATES[0])).field(acc.grib_fid(p))
        _, _, lat, lon, _ = grib2.grid_of(m)
        plans[p.native_grid] = acc.regrid_plan(p, (f.nj, f.ni), lat[::-1] if f.south_to_north else lat, lon)
    of = lambda kind: [(acc.parameter_namer(p), p.grib_name, acc.grib_fid(p), p.native_grid) for p in ds.params if p.kind == kind]  # noqa: E731
    stats = ds.stats if standardize else None
    T_in = ds.settings.num_input_steps
    io = load_titan_grib_batch(root, of("input_output"), [s.timestamps.validity_times for s in samples], stats, T_in, None, plans,
                               device=device, standardize=standardize)
    out_dates = [s.output_timestamps.validity_times for s in samples]
    ext = load_titan_grib_batch(root, of("input"), out_dates, stats, len(out_dates[0]), None, plans, device=device,
                                standardize=standardize).inputs.tensor
    table = torch.cat([forcings.time_table([s.timestamps.datetime], list(s.output_timestamps.timedeltas)) for s in samples])
    H, W = ds.grid.x, ds.grid.y
    gen = ops.build_forcing(None, None, None, table.to(device), forcings.grid_tables(ds.grid.lat, ds.grid.lon, device), len(samples),
                            table.shape[1], H, W)
    return io.inputs.tensor, io.outputs.tensor, torch.cat([ext, gen], dim=-1)


def _check(batch, want, names_io, names_ext):
    from py4cast_amd import forcings

    for got, ref in zip((batch.inputs.tensor, batch.outputs.tensor, batch.forcing.tensor), want):
        assert got.shape == ref.shape and torch.equal(got, ref) and bool(torch.isfinite(got).all())
    assert batch.inputs.feature_names == batch.outputs.feature_names == names_io
    assert batch.forcing.feature_names == names_ext + forcings.FORCING_NAMES


@pytest.mark.parametrize("prefetch,threads", [(0, 1), (0, 4), (2, 1), (2, 4)])
def test_the_loader_equals_the_whole_stream_route(prefetch, threads, gpu_device, tmp_path):
    from py4cast_amd.datasets import DeviceLoader

    ds = _dataset(tmp_path)
    assert len(ds) == 3
    with DeviceLoader(ds, batch_size=2, shuffle=False, prefetch=prefetch, threads=threads, device=gpu_device) as loader:
        for epoch in range(2):                                                       # the second epoch reuses the slots and the file index
            batches = list(loader)
            assert [b.inputs.tensor.shape for b in batches] == [(2, 2, 19, 23, 2), (1, 2, 19, 23, 2)]      # a short last batch
            for k, batch in enumerate(batches):
                _check(batch, _expected(ds, ds.sample_list[2 * k:2 * k + 2], gpu_device), ["aro_a_850hpa", "aro_a_500hpa"], ["arp_b_2m"])
            # per batch: the input_output group through the window kernel, the forcing group through unpack + regrid
            assert loader.routes.counts == {"window": 2 * (epoch + 1), "regrid": 2 * (epoch + 1)}
        # AROME.grib of all five dates, ARPEGE.grib of the three prediction dates (forcings are read at the prediction steps): once each
        assert loader.routes.files.parsed == 8 and all(b.is_pinned() for b in loader.buffers)
        assert float(batches[0].inputs.tensor.std()) > 0.01
    torch.cuda.synchronize()


def test_a_bitmap_sends_the_group_the_old_way(gpu_device, tmp_path):
    from py4cast_amd.datasets import DeviceLoader

    ds = _dataset(tmp_path, bitmap=True)
    with DeviceLoader(ds, batch_size=2, shuffle=False, prefetch=1, threads=2, device=gpu_device) as loader:
        for k, batch in enumerate(loader):
            _check(batch, _expected(ds, ds.sample_list[2 * k:2 * k + 2], gpu_device), ["aro_a_850hpa", "aro_a_500hpa"], ["arp_b_2m"])
        assert loader.routes.counts == {"window": 0, "regrid": 4}


def test_the_window_route_can_be_switched_off_and_changes_nothing(gpu_device, tmp_path):
    from py4cast_amd.datasets import DeviceLoader

    ds = _dataset(tmp_path)
    ds.settings.standardize = False
    got = {}
    for use in (True, False):
        with DeviceLoader(ds, batch_size=3, shuffle=False, prefetch=0, threads=2, device=gpu_device) as loader:
            it = iter(loader)
            loader.routes.use_window = use
            got[use] = next(it)
            assert loader.routes.counts == ({"window": 1, "regrid": 1} if use else {"window": 0, "regrid": 2})
            it.close()
    for part in ("inputs", "outputs", "forcing"):
        assert torch.equal(getattr(got[True], part).tensor, getattr(got[False], part).tensor)
    _check(got[True], _expected(ds, ds.sample_list, gpu_device, standardize=False), ["aro_a_850hpa", "aro_a_500hpa"], ["arp_b_2m"])


def test_conversion_to_npy_gives_the_batches_of_the_grib_loader(gpu_device, tmp_path, capsys):
    from py4cast_amd import diskio
    from py4cast_amd.datasets import DeviceLoader

    ds = _dataset(tmp_path)
    keep = (ds.settings.file_format, ds.settings.standardize)
    written = diskio.convert_titan_grib_to_npy(ds, device=gpu_device, batch=2)
    assert len(written) == 15 and all(p.exists() for p in written) and (ds.settings.file_format, ds.settings.standardize) == keep
    assert str(written[0]).endswith("subdatasets/titan_PAAROME_1S40_4-23-6-29/data/2023-03-01_00h00/aro_a_850hpa.npy")
    mtimes = [p.stat().st_mtime_ns for p in written]
    assert diskio.convert_titan_grib_to_npy(ds, device=gpu_device) == [] and [p.stat().st_mtime_ns for p in written] == mtimes
    npy = wc.titan_datasets(tmp_path, "npy", steps=STEPS)[0]
    assert len(npy) == 3
    batches = {}
    for name, d in (("grib", ds), ("npy", npy)):
        d.settings.standardize = False
        with DeviceLoader(d, batch_size=2, shuffle=False, prefetch=1, threads=2, device=gpu_device) as loader:
            batches[name] = list(loader)
    for a, b in zip(batches["grib"], batches["npy"]):
        for part in ("inputs", "outputs", "forcing"):
            assert torch.equal(getattr(a, part).tensor, getattr(b, part).tensor), part
            assert getattr(a, part).feature_names == getattr(b, part).feature_names
    assert len(batches["npy"]) == 2 and float(batches["npy"][0].inputs.tensor.mean()) > 1.0      # raw values, not standardised
    # a date whose file lacks the message: the reference's warning, the date skipped, the others written
    other = tmp_path / "broken"
    ds2 = _dataset(other)
    bad = diskio.titan_grib_path(other, "ARPEGE.grib", DATES[3])
    bad.write_bytes(diskio.titan_grib_path(other, "AROME.grib", DATES[3]).read_bytes())
    capsys.readouterr()
    written = diskio.convert_titan_grib_to_npy(ds2, device=gpu_device)
    said = capsys.readouterr().out
    assert "WARNING: Could not load grib arp_b_2m 2 2023-03-01 03:00:00. Skipping." in said
    assert len(written) == 12 and not any("03h00" in str(p) for p in written)
    torch.cuda.synchronize()
