"""
``TitanAccessor`` with ``file_format: grib`` without a GPU: paths, the numeric keys of a parameter's message, the sample enumeration
against the ``.npy`` tree of the same dates, and the host half of the loader's routes (``datasets.GribRoutes.layout`` / ``copy``): which
group goes which way and which bytes are copied.  The tree (tests/grib_window_cases.py): two GRIB files per date, three dates, one
parameter on the target grid at two levels and one on a coarser, PA_01D-like grid.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import datasets_fixtures as DF  # noqa: E402
import grib_window_cases as wc  # noqa: E402


def _npy_tree(root, ds, dates):
    for p in ds.params:
        for date in dates:
            from py4cast_amd import diskio

            path = diskio.titan_plane_path(ds.accessor.get_dataset_path("titan", ds.grid), p.name, p.level, p.level_type, date)
            path.parent.mkdir(parents=True, exist_ok=True)
            np.save(path, np.zeros((ds.grid.x, ds.grid.y), dtype=np.float32))


def test_grib_enumerates_the_samples_of_the_npy_tree(tmp_path):
    wc.write_titan_tree(tmp_path)
    grib = wc.titan_datasets(tmp_path, "grib")
    for ds in grib:
        assert ds.settings.file_format == "grib" and len(ds) == 2                    # this raised NotImplementedError before
    npy = wc.titan_datasets(tmp_path, "npy")
    _npy_tree(tmp_path, npy[0], wc.TITAN_DATES)
    assert DF.stamps_of(grib[0]) == DF.stamps_of(npy[0]) and len(npy[0]) == 2
    assert [s.timestamps.validity_times for s in grib[0].sample_list] == [wc.TITAN_DATES[:2], wc.TITAN_DATES[1:]]
    assert grib[0].grid.full_size == (wc.NJ, wc.NI) and (grib[0].grid.x, grib[0].grid.y) == (19, 23)


def test_a_sample_with_a_missing_file_is_dropped(tmp_path):
    wc.write_titan_tree(tmp_path, skip={(wc.TITAN_DATES[2], "ARPEGE.grib")})
    ds = wc.titan_datasets(tmp_path, "grib")[0]
    assert [s.timestamps.validity_times for s in ds.sample_list] == [wc.TITAN_DATES[:2]]
    arp = next(p for p in ds.params if p.name == "arp_b")
    import datetime as dt

    from py4cast_amd.datasets import Timestamps

    assert not ds.accessor.exists("titan", arp, Timestamps(wc.TITAN_DATES[2], [dt.timedelta(0)]), "grib")
    assert ds.accessor.exists("titan", arp, Timestamps(wc.TITAN_DATES[1], [dt.timedelta(0)]), "grib")


def test_paths_and_keys(tmp_path):
    from py4cast_amd import datasets as D
    from py4cast_amd import outputs

    wc.write_titan_tree(tmp_path)
    ds = wc.titan_datasets(tmp_path, "grib")[0]
    acc = ds.accessor
    a850, a500, arp = ds.params
    stamps = ds.sample_list[0].timestamps
    assert [str(p) for p in acc.paths("titan", a850, stamps, "grib")] == [
        str(tmp_path / "grib" / "2023-03-01_00h00" / "AROME.grib"), str(tmp_path / "grib" / "2023-03-01_01h00" / "AROME.grib")]
    assert str(acc.paths("titan", arp, stamps, "grib")[0]).endswith("grib/2023-03-01_00h00/ARPEGE.grib")
    assert acc.exists("titan", arp, stamps, "grib") and not acc.exists("titan", arp, stamps, "npy")
    assert str(acc.paths("titan", a850, stamps, "npy")[0]).endswith("subdatasets/titan_PAAROME_1S40_4-23-6-29/data/2023-03-01_00h00/aro_a_850hpa.npy")
    with pytest.raises(NotImplementedError):
        acc.paths("titan", a850, stamps, "netcdf")
    # grib_keys without a level take the parameter's; one that names its level keeps it
    assert acc.grib_fid(a850) == {"discipline": 0, "parameterCategory": 0, "parameterNumber": 0, "typeOfFirstFixedSurface": 100, "level": 850}
    assert acc.grib_fid(a500)["level"] == 500 and acc.grib_fid(arp)["level"] == 2
    assert "level" not in acc.metadata["WEATHER_PARAMS"]["aro_a"]["grib_keys"]         # the metadata itself is not touched
    # without grib_keys: the keys outputs.grib_fid knows for the feature name ...
    meta = wc.titan_metadata()
    meta["WEATHER_PARAMS"]["aro_t2m"] = dict(meta["WEATHER_PARAMS"]["arp_b"], grib="AROME.grib", grid="PAAROME_1S40", name="aro_t2m")
    del meta["WEATHER_PARAMS"]["aro_t2m"]["grib_keys"]
    acc2 = D.TitanAccessor(root=tmp_path, metadata=meta)
    t2m = D.WeatherParam("aro_t2m", 2, ds.grid, acc2.load_param_info, "input_output", acc2.get_weight_per_level)
    assert acc2.grib_fid(t2m) == outputs.grib_fid("aro_t2m_2m", 3600)[0] and acc2.grib_fid(t2m)
    # ... keys that are not matched are refused ...
    meta["WEATHER_PARAMS"]["aro_a"]["grib_keys"] = {"shortName": "t"}
    with pytest.raises(ValueError, match="aro_a.*shortName"):
        D.TitanAccessor(root=tmp_path, metadata=meta).grib_fid(a850)


def test_a_parameter_without_keys_is_refused_by_name_when_the_dataset_is_built(tmp_path):
    wc.write_titan_tree(tmp_path)
    with pytest.raises(ValueError, match="parameter aro_a .*grib_keys"):
        wc.titan_datasets(tmp_path, "grib", keys=False)
    three = wc.titan_datasets(tmp_path, "npy", keys=False)                           # the .npy format needs none
    assert len(three) == 3


def test_the_routes_of_a_batch(tmp_path):
    """the input_output group (on the target grid, no bitmap) is laid out as window slices, the forcing group (coarser grid) as whole
    streams; with a bitmap on one field of the target grid its whole group goes the old way"""
    from py4cast_amd import datapipe
    from py4cast_amd import datasets as D

    wc.write_titan_tree(tmp_path)
    ds = wc.titan_datasets(tmp_path, "grib")[0]
    routes = D.GribRoutes(ds)
    io = [p for p in ds.params if p.kind == "input_output"]
    ext = [p for p in ds.params if p.kind == "input"]
    dates = [s.timestamps.validity_times for s in ds.sample_list]                    # the two samples share a date
    lay = routes.layout(io, ["a850", "a500"], dates)
    assert lay.window and lay.start == 0 and lay.end % 4 == 0 and routes.files.parsed == 3
    plan = lay.plans[0]
    assert plan.identity and plan.out_shape == (19, 23) and lay.plans[1] is plan
    rows = datapipe.window_rows(plan)
    assert rows == (wc.NJ - 23, wc.NJ - 4)
    assert len(lay.copies) == 6                                                      # 2 levels x 3 distinct dates: the shared date once
    buf = np.full(lay.end + 8, 0xEE, dtype=np.uint8)
    for c in lay.copies:
        D.GribRoutes.copy(buf, *c)
    whole = 0
    for fi in range(2):
        for b in range(2):
            for t in range(2):
                _, _, f = lay.entries[fi][b][t]
                off, n, bit0 = lay.where[fi][b][t]
                first = bit0 // 8
                assert off % 4 == 0 and bit0 % 32 == 0 and n < len(f.stream) * 0.72     # 19 of 29 rows
                assert bytes(buf[off:off + n]) == bytes(f.stream[first:first + n])
                whole += len(f.stream)
    assert (buf[lay.end:] == 0xEE).all() and lay.end < 0.75 * whole * 6 / 8
    assert lay.where[0][0][1] == lay.where[0][1][0]                                  # sample 0's second date is sample 1's first
    table = datapipe.window_table([[[e[2] for e in pb] for pb in pf] for pf in lay.entries], lay.where, lay.names, plan)
    assert (table.fields["row_step"] == 1).all()                                     # a south-to-north file under the flipped plan
    lay2 = routes.layout(ext, ["b"], [s.output_timestamps.validity_times for s in ds.sample_list], at=lay.end)
    assert not lay2.window and lay2.start == lay.end and not lay2.plans[0].identity and lay2.plans[0].src_shape == (wc.ARP_NJ, wc.ARP_NI)
    assert all(c[2] == 0 and c[3] == len(c[1]) for c in lay2.copies) and len(lay2.copies) == 2
    routes.use_window = False
    assert not routes.layout(io, ["a850", "a500"], dates).window
    # a bitmap on the 500 hPa field: no random access, the group as a whole goes through unpack + regrid
    other = tmp_path / "masked"
    wc.write_titan_tree(other, bitmap=True)
    ds2 = wc.titan_datasets(other, "grib")[0]
    lay3 = D.GribRoutes(ds2).layout(io, ["a850", "a500"], dates)
    assert not lay3.window and len(lay3.copies) == 9 and lay3.plans[0].identity     # 6 streams and 3 bitmaps
    with pytest.raises(D.GribReadError, match="2001-03-01_00h00/AROME.grib: FileNotFoundError") as err:
        D.GribRoutes(ds2).layout(io, ["a850", "a500"], [[wc.TITAN_DATES[0].replace(year=2001)]])
    assert err.value.param is io[0] and isinstance(err.value, D.PlaneReadError)


def test_a_date_on_another_grid_is_refused_by_file(tmp_path):
    """every field of a parameter lies on one grid: the plan, the pitch of its planes and its crop come from the first one.  A later
    date of the same size but another origin (the window route would decode it with the wrong latitudes), of another size on the
    regrid route (its plane would not fit its pitch), and a message that is missing are refused with the file's name; so is a grid
    that changes from one sample to the next, whichever date comes first"""
    import numpy as np

    from py4cast_amd import datasets as D
    from py4cast_amd.diskio import titan_grib_path

    wc.write_titan_tree(tmp_path)
    ds = wc.titan_datasets(tmp_path, "grib")[0]
    io = [p for p in ds.params if p.kind == "input_output"]
    ext = [p for p in ds.params if p.kind == "input"]
    dates = [s.timestamps.validity_times for s in ds.sample_list]
    g = np.random.default_rng(9)
    good = D.GribRoutes(ds)
    assert good.layout(io, ["a850", "a500"], dates).window and not good.layout(ext, ["b"], dates).window
    # AROME.grib of the last date: the same 29 x 37 points one row further north
    moved = titan_grib_path(tmp_path, "AROME.grib", wc.TITAN_DATES[2])
    moved.write_bytes(b"".join(wc._grid_message(g, wc.NJ, wc.NI, wc.LAT_N + wc.GRID_STEP, wc.LON_W, wc.GRID_STEP, 16, 0, 0, 100, level,
                                                south_to_north=True) for level in (850, 500)))
    for use_window in (True, False):
        routes = D.GribRoutes(ds)
        routes.use_window = use_window
        with pytest.raises(D.GribReadError, match="2023-03-01_02h00/AROME.grib: aro_a_850hpa is on a grid of 29 x 37 whose latitudes") as err:
            routes.layout(io, ["a850", "a500"], dates)
        assert err.value.param is io[0] and "2023-03-01_00h00/AROME.grib" in str(err.value)
        with pytest.raises(D.GribReadError, match="2023-03-01_01h00/AROME.grib"):        # the odd one first: the next date is named
            routes.layout(io, ["a850", "a500"], [dates[1][::-1]])
        assert routes.layout(io, ["a850", "a500"], dates[:1]).plans[0].identity            # the dates before it still load
    # ARPEGE.grib of the middle date: two more rows and columns
    wider = titan_grib_path(tmp_path, "ARPEGE.grib", wc.TITAN_DATES[1])
    wider.write_bytes(wc._grid_message(g, wc.ARP_NJ + 2, wc.ARP_NI + 2, wc.LAT_N + 2 * wc.ARP_STEP, wc.LON_W - 2 * wc.ARP_STEP, wc.ARP_STEP, 16, 1, 1, 103, 2))
    with pytest.raises(D.GribReadError, match="2023-03-01_01h00/ARPEGE.grib: arp_b_2m is on a grid of 20 x 24") as err:
        D.GribRoutes(ds).layout(ext, ["b"], dates)
    assert err.value.param is ext[0]
    # a file without the message: named with the keys that were looked for
    wider.write_bytes(moved.read_bytes())
    with pytest.raises(D.GribReadError, match="2023-03-01_01h00/ARPEGE.grib: KeyError.*parameterCategory"):
        D.GribRoutes(ds).layout(ext, ["b"], dates)


def test_the_loader_refuses_the_host_for_grib(tmp_path):
    from py4cast_amd import datasets as D

    wc.write_titan_tree(tmp_path)
    ds = wc.titan_datasets(tmp_path, "grib")[0]
    with pytest.raises(ValueError, match="no host path"):
        iter(D.DeviceLoader(ds, batch_size=2, device="cpu"))
