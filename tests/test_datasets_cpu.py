"""
py4cast_amd/datasets.py on the host against the fixtures the unmodified reference wrote (tests/golden/make_golden_datasets.py):
periods, the sample enumeration, the statics (bit for bit), the DatasetInfo, the accessors' paths and readers, and the
DeviceLoader on the CPU device, whose batches are the host statement of the device kernels.
"""
import datetime as dt
import json
import os
import warnings
import zipfile

import numpy as np
import pytest
import torch

import datasets_fixtures as DF


def D():
    from py4cast_amd import datasets

    return datasets


# ------------------------------------------------------------------------------------------ periods and enumeration
@pytest.mark.parametrize("form", ("obs", "refcst"))
def test_period_pairs_equal_the_reference(form):
    with open(os.path.join(DF.GOLD, "datasets_periods.json")) as f:
        want = json.load(f)[form]
    p = D().Period(name="train", **want["kwargs"])
    got = [[t0.strftime("%Y-%m-%dT%H:%M:%S"), int(lt.total_seconds())] for t0, lt in p.available_t0_and_leadtimes]
    assert got == want["pairs"] and p.forecast_step.total_seconds() == want["forecast_step"]
    assert all(isinstance(t0, dt.datetime) and isinstance(lt, dt.timedelta) for t0, lt in p.available_t0_and_leadtimes)


def test_period_needs_one_of_the_two_forms():
    with pytest.raises(ValueError, match="obs_step"):
        D().Period(name="train", start=20230101, end=20230102)
    p = D().Period(name="x", start=20230101, end=20230101, obs_step=3600)
    assert p.obs_step_btw_t0 == p.obs_step == dt.timedelta(hours=1)


def test_timestamps_validity_times():
    t = D().Timestamps(dt.datetime(2023, 1, 1, 3), [dt.timedelta(hours=-1), dt.timedelta(0), dt.timedelta(hours=2)])
    assert t.validity_times == [dt.datetime(2023, 1, 1, 2), dt.datetime(2023, 1, 1, 3), dt.datetime(2023, 1, 1, 5)]


@pytest.mark.parametrize("steps,key", (((1, 1, 1), "obs_1_1"), ((2, 3, 3), "obs_2_3")))
def test_observation_enumeration_equals_the_reference(tmp_path, steps, key, capsys):
    with open(os.path.join(DF.GOLD, "datasets_samples.json")) as f:
        want = json.load(f)[key]
    train, valid, test = D().NativeDataset.from_dict(D().DummyAccessor(root=tmp_path), "dummy", DF.confs()["dummy"], *steps)
    assert DF.stamps_of(train) == want and len(train) == len(want)
    assert f"--> {len(want)} train samples are now defined, with 0 invalid samples." in capsys.readouterr().out
    assert valid.settings.num_pred_steps == steps[2] and train.settings.num_pred_steps == steps[1] and test.period.name == "test"


@pytest.mark.parametrize("name", ("poesy", "rainfall", "titan"))
def test_enumeration_on_files_equals_the_reference(tmp_path, name, capsys):
    ds, _, _, meta = DF.build(name, tmp_path)
    assert DF.stamps_of(ds) == meta["samples"] and len(ds) == meta["len"]
    out = capsys.readouterr().out
    assert f"--> {meta['len']} {ds.period.name} samples are now defined, with" in out and "with 0 invalid" not in out


def test_poesy_validity_check_at_both_ends_of_terms(tmp_path):
    ds, _, _, meta = DF.build("poesy", tmp_path)
    acc, step = ds.accessor, dt.timedelta(hours=3)
    t0 = dt.datetime(2021, 6, 15, 3)
    ok = lambda lead, n_in=2, n_pred=2: acc.optional_check_before_exists(t0, n_in, n_pred, step, dt.timedelta(hours=lead))  # noqa: E731
    assert not ok(3) and ok(4) and ok(39) and not ok(40)          # lead - 3 h >= 1 h and lead + 6 h <= 45 h
    assert ok(1, 1, 1) and not ok(0, 1, 1) and ok(42, 1, 1) and not ok(43, 1, 1)
    leads = sorted({s["timedeltas"][1] // 3600 for s in meta["samples"]})
    assert leads[0] == 6 and leads[-1] == 39


@pytest.mark.parametrize("name", ("rainfall", "titan", "poesy"))
def test_a_missing_file_drops_exactly_that_sample(tmp_path, name):
    ds, three, _, meta = DF.build(name, tmp_path)
    victim = ds.sample_list[1]
    path = ds.accessor.paths(ds.settings.dataset_name, ds.params[0], victim.timestamps, ds.settings.file_format)[-1]
    os.remove(path)
    again = D().NativeDataset(ds.name, ds.grid, ds.period, ds.params, ds.settings, ds.accessor)
    gone = [s for s in meta["samples"] if not any(DF.stamps_of(again)[i] == s for i in range(len(again)))]
    readers = [s for s in ds.sample_list if str(path) in map(str, ds.accessor.paths(ds.settings.dataset_name, ds.params[0], s.timestamps,
                                                                                   ds.settings.file_format))]
    assert len(gone) == len(readers) >= 1 and len(again) == len(ds) - len(readers)
    assert {g["datetime"] for g in gone} == {s.timestamps.datetime.strftime("%Y-%m-%dT%H:%M:%S") for s in readers}


# ------------------------------------------------------------------------------------------ grid and statics
def _grid(border, geo=None):
    z = np.load(os.path.join(DF.GOLD, "datasets_statics.npz"))
    gp = z["geopotential"] if geo is None else geo
    return z, D().Grid(name="g", load_grid_info_func=lambda n: D().GridConfig((5, 7), z["lat"], z["lon"], gp, None), border_size=border)


@pytest.mark.parametrize("key,border", (("border0", 0), ("border1", 1)))
def test_statics_bit_equal(key, border):
    z, grid = _grid(border)
    nt = D().grid_static_features(grid, [])
    assert nt.feature_names == [str(n) for n in z[f"{key}_names"]] and nt.names == ["lat", "lon", "features"]
    assert nt.tensor.dtype == torch.float32 and np.array_equal(nt.tensor.numpy().view(np.uint32), z[key].view(np.uint32))
    assert grid.grid_limits == list(z[f"{key}_limits"]) and grid.N_grid == 35 and (grid.x, grid.y) == (5, 7)
    assert grid.border_mask.sum() == (0 if border == 0 else 35 - 3 * 5) and grid.meshgrid.shape == (2, 5, 7)
    assert grid.lat.shape == grid.lon.shape == (5, 7) and grid.projection == ("PlateCarree", {})


def test_constant_geopotential_warns_and_becomes_one():
    z, grid = _grid(1, np.full((5, 7), 7.5))
    with pytest.warns(UserWarning, match="Geopotential is constant"):
        nt = D().grid_static_features(grid, [])
    assert np.array_equal(nt.tensor.numpy().view(np.uint32), z["constant"].view(np.uint32)) and bool((nt["geopotential"] == 1).all())


def test_negative_border_is_refused():
    _, grid = _grid(-1)
    with pytest.raises(ValueError, match="Bordersize"):
        grid.border_mask


@pytest.mark.parametrize("name", DF.ACCESSORS)
def test_dataset_info_equals_the_reference(tmp_path, name):
    from py4cast_amd import base

    ds, _, arrays, meta = DF.build(name, tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        info = ds.dataset_info
    assert isinstance(info, base.DatasetInfo) and isinstance(info.statics, base.Statics) and isinstance(info.stats, base.Stats)
    assert info.name == meta["name"] and (info.weather_dim, info.forcing_dim) == (meta["weather_dim"], meta["forcing_dim"])
    assert (ds.weather_dim, ds.forcing_dim) == (meta["weather_dim"], meta["forcing_dim"])
    assert info.pred_step.total_seconds() == meta["pred_step"] and info.shortnames == meta["shortnames"] and info.units == meta["units"]
    assert info.state_weights == meta["state_weights"]
    # rainfall's limits are projected corners: two float64 evaluations of the closed form (test_rainfall_projection_corners)
    assert np.allclose(info.domain_info.grid_limits, meta["grid_limits"], rtol=0, atol=1e-6 if name == "rainfall" else 0)
    assert info.statics.grid_statics.feature_names == meta["statics_names"]
    assert np.array_equal(info.statics.grid_statics.tensor.numpy().view(np.uint32), arrays["statics"].view(np.uint32))
    for n, st in meta["stats"].items():
        assert float(info.stats[n]["mean"]) == float(np.float32(st["mean"])) and float(info.diff_stats[n]["std"]) == float(np.float32(meta["diff_stats"][n]["std"]))


# ------------------------------------------------------------------------------------------ registry, paths, readers
def test_registry_resolves_by_substring(tmp_path):
    d = D()
    assert d.resolve_accessor("Poesy") is d.PoesyAccessor and d.resolve_accessor("titan_refacto") is d.TitanAccessor
    assert d.resolve_accessor("my_rainfall_v2") is d.RainfallAccessor and d.resolve_accessor("dummy") is d.DummyAccessor
    assert d.resolve_accessor("titan_dummy") is d.TitanAccessor            # the first registered key wins
    with pytest.raises(ValueError, match="registry substring"):
        d.resolve_accessor("era5")
    train, _, _ = d.get_datasets("a_dummy_run", 1, 1, 1, DF.confs()["dummy"], root=tmp_path)
    assert isinstance(train.accessor, d.DummyAccessor) and str(train) == "a_dummy_run_dummygrid"
    with pytest.raises(TypeError, match="instance"):
        d.NativeDataset.from_dict(d.DummyAccessor, "dummy", DF.confs()["dummy"], 1, 1, 1)


def test_accessor_paths(tmp_path):
    d, c = D(), DF.confs()
    stamps = d.Timestamps(dt.datetime(2024, 1, 1, 3), [dt.timedelta(minutes=-5), dt.timedelta(0)])
    rain = d.RainfallAccessor(root="/data/rain")
    g = d.Grid(name="rainfallgrid", load_grid_info_func=rain.load_grid_info, border_size=0, subdomain=(0, 16, 0, 16))
    p = d.WeatherParam("precip", 0, g, rain.load_param_info, "input_output", rain.get_weight_per_level)
    assert [str(x) for x in rain.paths("rainfall", p, stamps, "npz")] == ["/data/rain/Hexagone/2024/202401010255.npz",
                                                                        "/data/rain/Hexagone/2024/202401010300.npz"]
    assert rain.parameter_namer(p) == "precip" and p.state_weight == 1.0 and p.level_type == "surface" and p.unit == "mm/h"
    assert p.parameter_name == "lame d'eau Serval_0_surface" and rain.transform(p, "npz") == (0.0, 100.0, 12.0, True)
    assert g.full_size == (1536, 1536) and bool((g.geopotential == 1).all())

    DF.write_files("titan", str(tmp_path))
    titan = d.TitanAccessor(root=tmp_path, metadata=c["titan_metadata"])
    tg = d.Grid(name="PAAROME_1S100", load_grid_info_func=titan.load_grid_info, border_size=2, subdomain=(0, 12, 0, 9))
    t2m = d.WeatherParam("aro_t2m", 2, tg, titan.load_param_info, "input_output", titan.get_weight_per_level)
    t850 = d.WeatherParam("aro_t", 850, tg, titan.load_param_info, "input_output", titan.get_weight_per_level)
    assert titan.parameter_namer(t2m) == "aro_t2m_2m" and titan.parameter_namer(t850) == "aro_t_850hpa"
    assert t2m.state_weight == 2.0 and t850.state_weight == 1 + 850 / 1000 and t850.level_type == "isobaricInhPa"
    assert str(titan.paths("titan", t850, stamps, "npy")[0]) == str(
        tmp_path / "subdatasets" / "titan_PAAROME_1S100_0-12-0-9" / "data" / "2024-01-01_02h55" / "aro_t_850hpa.npy")
    assert tg.lat.shape == (12, 9) and tg.lat[0, 0] > tg.lat[-1, 0] and np.isfinite(tg.geopotential).all()
    with pytest.raises(NotImplementedError):
        titan.load_grid_info("EURW1S40")

    poesy = d.PoesyAccessor(root="/data/poesy", metadata=c["poesy_metadata"])
    pp = d.WeatherParam("tirf", 0, tg, poesy.load_param_info, "input_output", poesy.get_weight_per_level)
    assert str(poesy.paths("poesy", pp, stamps, "npy")[0]) == "/data/poesy/2024-01-01T03:00:00Z_rrdecum_lt1-45_crop.npy"
    assert pp.state_weight == 1.0 and str(poesy.cache_dir("poesy", tg)) == "/data/poesy/cache/poesy_PAAROME_1S100"
    with pytest.raises(ValueError, match="metadata"):
        d.PoesyAccessor(root="/data/poesy")


def test_rainfall_projection_corners():
    d = D()
    with open(os.path.join(DF.GOLD, "datasets_rainfall_corners.json")) as f:
        corners = json.load(f)["corners"]
    assert set(corners) == set(d.RAINFALL_DOMAIN)
    for name, c in corners.items():
        x, y = d.stereographic_forward(c["lon"], c["lat"])
        # two float64 evaluations of one closed form through different intermediates: a few ulp of 1e6 m
        assert abs(x - c["x"]) < 1e-6 and abs(y - c["y"]) < 1e-6, (name, x - c["x"], y - c["y"])
    # what the closed form must satisfy whatever its spelling: the centre maps to the origin, the central meridian to x = 0, and the
    # scale there is 1 -- a step of 1e-6 degrees northwards is the meridian arc M(45) * dphi
    x0, y0 = d.stereographic_forward(0.0, 45.0)
    assert abs(x0) < 1e-9 and abs(y0) < 1e-9 and abs(d.stereographic_forward(0.0, 50.0)[0]) < 1e-9
    e2 = d.WGS84_F * (2 - d.WGS84_F)
    M = d.WGS84_A * (1 - e2) / (1 - e2 * np.sin(np.radians(45.0)) ** 2) ** 1.5
    assert abs(d.stereographic_forward(0.0, 45.0 + 1e-6)[1] / (M * np.radians(1e-6)) - 1) < 1e-6
    minx, maxx, miny, maxy = d.rainfall_extent()
    assert (minx, maxx, miny, maxy) == (corners["lower_left"]["x"], corners["lower_right"]["x"], corners["lower_left"]["y"],
                                       corners["upper_right"]["y"]) or max(abs(minx - corners["lower_left"]["x"]), abs(maxy - corners["upper_right"]["y"])) < 1e-6
    cfg = d.RainfallAccessor(root="/x").load_grid_info("rainfallgrid")
    assert cfg.latitude[0] == maxy and cfg.latitude[-1] == miny and cfg.longitude[0] == minx and len(cfg.latitude) == 1536


def test_npz_reader(tmp_path):
    d = D()
    a = (np.arange(12 * 9, dtype=np.int16) - 50).reshape(12, 9)
    np.savez(tmp_path / "stored.npz", a)
    np.savez_compressed(tmp_path / "deflated.npz", a)
    with zipfile.ZipFile(tmp_path / "stored.npz") as z:
        assert z.getinfo("arr_0.npy").compress_type == zipfile.ZIP_STORED
    with zipfile.ZipFile(tmp_path / "deflated.npz") as z:
        assert z.getinfo("arr_0.npy").compress_type == zipfile.ZIP_DEFLATED
    for name in ("stored.npz", "deflated.npz"):
        dst = np.zeros((12, 9), np.int16)
        d.read_npz_plane(tmp_path / name, dst)
        assert np.array_equal(dst, a) and d.npy_header(tmp_path / name) == ((12, 9), np.dtype("<i2"))
    with pytest.raises(ValueError, match="expected"):
        d.read_npz_plane(tmp_path / "stored.npz", np.zeros((9, 12), np.int16))
    with pytest.raises(ValueError, match="expected"):
        d.read_npz_plane(tmp_path / "stored.npz", np.zeros((12, 9), np.float32))
    # a member whose header promises more than it holds
    import io

    buf = io.BytesIO()
    np.save(buf, a)
    with zipfile.ZipFile(tmp_path / "short.npz", "w") as z:
        z.writestr("arr_0.npy", buf.getvalue()[:-40])
    with pytest.raises(ValueError, match="truncated"):
        d.read_npz_plane(tmp_path / "short.npz", np.zeros((12, 9), np.int16))
    with zipfile.ZipFile(tmp_path / "other.npz", "w") as z:
        z.writestr("arr_1.npy", buf.getvalue())
    with pytest.raises(ValueError, match="no member"):
        d.read_npz_plane(tmp_path / "other.npz", np.zeros((12, 9), np.int16))
    np.save(tmp_path / "plane.npy", a.astype(np.float64))
    dst = np.zeros((12, 9), np.float64)
    d.read_npy_plane(tmp_path / "plane.npy", dst)
    assert np.array_equal(dst, a)


# ------------------------------------------------------------------------------------------ the loader on the CPU device
def _first_values(loader):
    return [b.inputs.tensor[:, 0, 0, 0, 0].tolist() for b in loader]


def test_loader_order_shuffle_seed_drop_last(tmp_path):
    d = D()
    ds, _, _, _ = DF.build("rainfall", tmp_path)
    n = len(ds)     # 7
    cpu = torch.device("cpu")
    plain = d.DeviceLoader(ds, batch_size=1, device=cpu, threads=2)
    per_sample = [v[0] for v in _first_values(plain)]
    assert len(plain) == n and len(per_sample) == n and len(set(per_sample)) > 1
    assert [v[0] for v in _first_values(plain)] == per_sample                 # a second epoch without shuffle: the same order
    with d.DeviceLoader(ds, batch_size=2, device=cpu, threads=4, prefetch=0) as two:
        got = _first_values(two)
        assert len(two) == 4 and [len(g) for g in got] == [2, 2, 2, 1] and [x for g in got for x in g] == per_sample
    with d.DeviceLoader(ds, batch_size=2, device=cpu, drop_last=True) as dropped:
        assert len(dropped) == 3 and [x for g in _first_values(dropped) for x in g] == per_sample[:6]
    a = d.DeviceLoader(ds, batch_size=3, shuffle=True, seed=5, device=cpu)
    b = d.DeviceLoader(ds, batch_size=3, shuffle=True, seed=5, device=cpu, prefetch=1, threads=1)
    c = d.DeviceLoader(ds, batch_size=3, shuffle=True, seed=6, device=cpu)
    e0, e1 = _first_values(a), _first_values(a)
    assert e0 == _first_values(b) and e1 == _first_values(b)               # the same seed: the same epochs
    assert a.order(0) == torch.randperm(n, generator=torch.Generator().manual_seed(5)).tolist() and a.order(1) != a.order(0)
    assert sorted(x for g in e0 for x in g) == sorted(per_sample) and e0 != e1 and a.order(0) != c.order(0)
    for loader in (plain, a, b, c):
        loader.close()


def test_loader_refuses_more_than_16_threads_and_names_the_broken_file(tmp_path):
    d = D()
    ds, _, _, _ = DF.build("rainfall", tmp_path)
    with pytest.raises(ValueError, match="17 threads"):
        d.DeviceLoader(ds, threads=17, device="cpu")
    d.DeviceLoader(ds, threads=16, device="cpu").close()
    victim = ds.accessor.paths("rainfall", ds.params[0], ds.sample_list[2].timestamps, "npz")[3]
    with open(victim, "r+b") as f:
        f.truncate(os.path.getsize(victim) - 64)
    with d.DeviceLoader(ds, batch_size=1, device="cpu", threads=4, prefetch=2) as loader:
        it = iter(loader)
        next(it), next(it)
        with pytest.raises(d.PlaneReadError, match=str(victim).replace(".", r"\.")):
            next(it)


@pytest.mark.parametrize("name", DF.ACCESSORS)
def test_loader_batches_equal_the_reference_on_the_cpu_device(tmp_path, name, capsys):
    d = D()
    ds, _, arrays, meta = DF.build(name, tmp_path)
    n = meta["n_samples"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with d.DeviceLoader(ds, batch_size=n, device="cpu", threads=4) as loader:
            batch = next(iter(loader))
            assert batch.inputs.tensor.shape[0] == n
            DF.check_batch(batch, arrays, meta, slice(0, n))
        with d.DeviceLoader(ds, batch_size=2, device="cpu", threads=1, prefetch=0) as loader:   # a ring of one buffer, reused
            for k, batch in zip(range(n // 2), loader):
                DF.check_batch(batch, arrays, meta, slice(2 * k, 2 * k + 2))


def test_statistics_dataloader_contract(tmp_path):
    """what dataset_stats reads of a dataset: ``torch_dataloader()`` yields batches with .inputs / .outputs / .forcing, and
    ``settings.standardize`` False gives the raw (transformed) values"""
    d = D()
    ds, _, arrays, meta = DF.build("rainfall", tmp_path)
    ds.settings.standardize = False
    batch = next(iter(ds.torch_dataloader(device="cpu")))
    raw = arrays["file::Hexagone/2024/202401010000.npz"]
    want = (np.where(raw < 0, 0, raw) / 100 * 12)[::-1]
    assert batch.inputs.tensor.shape == (1, 2, 16, 16, 1) and batch.outputs.tensor.shape[1] == 3
    assert np.allclose(batch.inputs.tensor[0, 1, :, :, 0].numpy(), want, rtol=3 * 2.0 ** -24, atol=0)
    ds.settings.standardize = True


def test_output_only_parameters_are_refused_as_the_reference_refuses_them(tmp_path):
    """base.py:455-527 appends an ``output`` parameter to the targets and the Item it builds then raises (base.py:98-113): the same
    error, before anything is read"""
    d = D()
    DF.write_files("titan", str(tmp_path))
    conf = json.loads(json.dumps(DF.confs()["titan"]))
    conf["params"]["aro_r2"]["kind"] = "output"
    train, _, _ = d.NativeDataset.from_dict(DF.accessor("titan", str(tmp_path)), "titan", conf, 1, 2, 2)
    with d.DeviceLoader(train, batch_size=1, device="cpu") as loader:
        with pytest.raises(ValueError, match="Inputs and outputs must have the same feature names"):
            next(iter(loader))
    conf["params"] = {"aro_r2": {"levels": [2], "kind": "input"}}
    train, _, _ = d.NativeDataset.from_dict(DF.accessor("titan", str(tmp_path)), "titan", conf, 1, 2, 2)
    with d.DeviceLoader(train, batch_size=1, device="cpu") as loader:
        with pytest.raises(ValueError, match="list of outputs is empty"):
            next(iter(loader))


def test_from_yaml_both_layouts(tmp_path):
    import yaml

    d = D()
    DF.write_files("rainfall", str(tmp_path / "data"))
    conf = DF.confs()["rainfall"]
    cli = tmp_path / "my_rainfall.yaml"        # the layout of config/CLI/dataset/*.yaml
    cli.write_text(yaml.safe_dump({"data": {"dataset_name": "rainfall", "num_input_steps": 2, "num_pred_steps_train": 1,
                                            "num_pred_steps_val_test": 3, "batch_size": 1, "dataset_conf": conf}}, sort_keys=False))
    train, valid, test = d.NativeDataset.from_yaml(cli, root=tmp_path / "data")
    _, meta = DF.golden("rainfall")
    assert isinstance(train.accessor, d.RainfallAccessor) and train.name == "rainfall" and str(train) == meta["name"]
    assert (train.settings.num_input_steps, train.settings.num_pred_steps, valid.settings.num_pred_steps) == (2, 1, 3)
    assert DF.stamps_of(valid) == meta["samples"] and test.period.name == "test"
    bare = tmp_path / "rainfall_bare.yaml"     # the dataset_conf mapping itself; the accessor given, the steps as arguments
    bare.write_text(yaml.safe_dump(conf, sort_keys=False))
    t2, v2, _ = d.NativeDataset.from_yaml(bare, accessor=d.RainfallAccessor(root=tmp_path / "data"), num_input_steps=2,
                                          num_pred_steps_train=1, num_pred_steps_val_test=3)
    assert t2.name == "rainfall_bare" and DF.stamps_of(v2) == meta["samples"]


def test_a_loader_without_a_device_is_refused_and_torch_dataloader_gives_its_threads_back(tmp_path):
    d = D()
    ds, _, _, _ = DF.build("rainfall", tmp_path)
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match='device="cpu"'):
            d.DeviceLoader(ds)
    loader = ds.torch_dataloader(device="cpu")
    for _ in loader:
        assert loader.pool is not None
    assert loader.pool is None and loader.groups is None          # closed when the epoch ended
    it = iter(loader)
    next(it)
    assert loader.pool is not None
    del it                                                       # an abandoned epoch (the statistics passes take one batch this way)
    assert loader.pool is None
