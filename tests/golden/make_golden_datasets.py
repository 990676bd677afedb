#!/usr/bin/env python3
"""
Golden fixtures for py4cast_amd/datasets.py -- runs ONLY in the build container (needs the reference).

Executes the unmodified reference files ``py4cast/datasets/{access,base,dummy,rainfall}.py``, ``datasets/poesy/__init__.py`` and
``datasets/titan/__init__.py`` through ``sys.modules`` stubs of what they import beside numpy and torch (recipe of
make_golden.py): a metadata-only NamedTensor, cartopy, xarray, skimage, gif, ``py4cast.plots`` / ``py4cast.utils``.  Where the
reference has a module-level data path (``SCRATCH_PATH``, ``CACHE_DIR``) or its packaged metadata, the loaded module's attribute
is pointed at a temporary directory / a trimmed copy; no reference file is edited.  Written next to this script:

* ``datasets_confs.json``: the tiny dataset configurations and the trimmed metadata the tests build their datasets from
  (settings only);
* ``datasets_periods.json``: ``Period.available_t0_and_leadtimes`` for both forms;
* ``datasets_samples.json``: the time stamps (and members) of ``DatasetABC.sample_list`` for (T_in, T) = (1, 1) and (2, 3) on a
  3-day observation period with ``obs_step_btw_t0`` != ``obs_step``, and for a 2-day poesy period with two daily runs whose lead
  times run past both ends of ``TERMS`` (and one run's file missing);
* ``datasets_statics.npz``: ``grid_static_features`` on a 5 x 7 grid with borders 0 and 1 and with a constant geopotential;
* ``datasets_load_{dummy,poesy,rainfall,titan}.npz``: the files the generator wrote for the accessor (``file::<relative path>``),
  the statistics, and ``collate_fn`` of ``Sample.load`` of the first samples -- with ``d_ref_date`` / ``d_ref_toa``, the reference's
  own worst deviation of the generated forcings from the float64 closed form (tests/forcing_closed_form.py), the unit of the
  tests' tolerance on those channels;
* ``datasets_rainfall_corners.json``: see ``rainfall_corners`` -- cartopy is absent and is NOT stubbed into giving numbers.

    python tests/golden/make_golden_datasets.py
"""

import datetime as dt
import importlib
import json
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import forcing_closed_form as cf  # noqa: E402
import grib2_reference as gr  # noqa: E402  (builds the conf_<grid>.grib of the titan fixture)
import make_golden as mg  # noqa: E402  (where the reference lies, the stub helper)


class NamedTensor(mg.NamedTensor):   # metadata only: the two calls Sample.load / collate_fn add to make_golden's shim
    def __init__(self, tensor, names, feature_names, feature_dim_name="features"):
        super().__init__(tensor, list(names), list(feature_names), feature_dim_name)

    def __getitem__(self, name):
        d = self.names.index("features")
        return self.tensor.select(d, self.feature_names_to_idx[name]).unsqueeze(d)

    def type_(self, dtype):
        self.tensor = self.tensor.type(dtype)

    @staticmethod
    def concat(nts):
        assert all(n.names == nts[0].names for n in nts)
        return NamedTensor(torch.cat([n.tensor for n in nts], dim=nts[0].names.index("features")), nts[0].names.copy(),
                           [f for n in nts for f in n.feature_names])

    def unsqueeze_and_expand_from_(self, other):
        sizes = []
        for i, name in enumerate(other.names):
            if name not in self.names:
                self.tensor = self.tensor.unsqueeze(i)
                self.names.insert(i, name)
                sizes.append(other.dim_size(name))
            else:
                sizes.append(-1)
        self.tensor = self.tensor.expand(*sizes)

    @staticmethod
    def expand_to_batch_like(tensor, other):
        return NamedTensor(tensor, ["batch"] + other.names, other.feature_names.copy())


class NoCartopy:
    """stands where cartopy's projections are named; asked for a number it refuses"""

    def __init__(self, *a, **k):
        pass

    def transform_point(self, *a, **k):
        raise RuntimeError("cartopy is absent: no projected coordinate can come from this stub")


def install(tmp: Path):
    os.environ["PY4CAST_ROOTDIR"] = str(tmp / "rootdir")
    os.environ["PY4CAST_TITAN_PATH"] = str(tmp / "titan")
    sys.path.insert(0, mg.REF)
    mg.stub("cartopy", crs=mg.stub("cartopy.crs", PlateCarree=NoCartopy, Stereographic=NoCartopy, LambertConformal=NoCartopy))
    mg.stub("mfai")
    mg.stub("mfai.pytorch")
    mg.stub("mfai.pytorch.namedtensor", NamedTensor=NamedTensor)
    mg.stub("gif", frame=lambda f: f)
    mg.stub("xarray", Dataset=object)
    mg.stub("skimage")
    mg.stub("skimage.transform", resize=None)
    mg.stub("py4cast.plots", DomainInfo=lambda **k: types.SimpleNamespace(**k))

    class RegisterFieldsMixin:
        pass

    mg.stub("py4cast.utils", RegisterFieldsMixin=RegisterFieldsMixin, merge_dicts=None, torch_save=torch.save)
    # access.py:325 annotates a field ``Callable[[int, str], [float]]``; typing before Python 3.11 refuses a list as the result type
    # at import.  The annotation is never evaluated again: let lists through for the duration of the imports.
    import typing

    strict = typing._type_check
    typing._type_check = lambda arg, msg, *a, **k: arg if isinstance(arg, list) else strict(arg, msg, *a, **k)
    try:
        mods = {n: importlib.import_module(f"py4cast.datasets.{n}") for n in ("access", "base", "dummy", "rainfall", "poesy", "titan")}
    finally:
        typing._type_check = strict
    return types.SimpleNamespace(**mods)


def iso(t):
    return t.strftime("%Y-%m-%dT%H:%M:%S")


def stamps_of(ds):
    return [{"datetime": iso(s.timestamps.datetime), "timedeltas": [int(d.total_seconds()) for d in s.timestamps.timedeltas],
             "member": int(s.member)} for s in ds.sample_list]


def write_json(name, obj):
    path = os.path.join(HERE, name)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1)     # key order is data: the parameters of a configuration come in it
    print(f"{name}: {os.path.getsize(path)} bytes")


def save_stats(path: Path, stats: dict):
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save({k: {s: torch.tensor(v) for s, v in d.items()} for k, d in stats.items()}, path)


def load_fixture(R, name, ds, files: dict, stats: dict, diff_stats: dict, n_samples: int, extra=None):
    """collate_fn of Sample.load of the first ``n_samples`` samples + everything the test needs to set the same dataset up"""
    samples = ds.sample_list[:n_samples]
    batch = R.base.collate_fn([s.load() for s in samples])
    out = {f"file::{k}": v for k, v in files.items()}
    for part in ("inputs", "outputs", "forcing"):
        nt = getattr(batch, part)
        assert nt.tensor.dtype == torch.float32 and nt.names == ["batch", "timestep", "lat", "lon", "features"]
        out[part] = nt.tensor.numpy()
        out[f"{part}_names"] = np.array(nt.feature_names)
    # the reference's own error on the generated forcings, per sample with its own lead times (fp32-rounded coordinates)
    lat, lon = ds.grid.lat.astype(np.float32), ds.grid.lon.astype(np.float32)
    gen = out["forcing"][..., -5:]
    d_date = d_toa = 0.0
    for b, s in enumerate(samples):
        want_date, _, want_toa = cf.batch(lat, lon, [s.timestamps.datetime], list(s.output_timestamps.timedeltas))
        d_date = max(d_date, float(np.abs(gen[b, :, 0, 0, :4] - want_date[0]).max()))
        d_toa = max(d_toa, float(np.abs(gen[b, ..., 4] - want_toa[0]).max()))
    info = ds.dataset_info
    meta = {"stats": stats, "diff_stats": diff_stats, "n_samples": n_samples, "len": len(ds), "name": str(ds),
            "weather_dim": info.weather_dim, "forcing_dim": info.forcing_dim, "pred_step": info.pred_step.total_seconds(),
            "shortnames": info.shortnames, "units": info.units, "state_weights": {k: float(v) for k, v in info.state_weights.items()},
            "statics_names": info.statics.grid_statics.feature_names, "grid_limits": list(ds.grid.grid_limits),
            "samples": stamps_of(ds), "d_ref_date": d_date, "d_ref_toa": d_toa}
    meta.update(extra or {})
    out["statics"] = info.statics.grid_statics.tensor.numpy()
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, f"datasets_load_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"datasets_load_{name}.npz: {os.path.getsize(path)} bytes, {len(ds)} samples, batch {tuple(out['outputs'].shape)}, "
          f"d_ref_date {d_date:.3g}, d_ref_toa {d_toa:.3g}")


def rainfall_corners():
    """The four projected corners of the rainfall domain.  cartopy is absent here and its stub refuses to produce numbers, so
    the corners are pinned against the closed form instead: the ellipsoidal oblique stereographic projection (WGS84, scale factor
    1 at latitude 45, longitude 0) written with the isometric latitude psi = atanh(sin phi) - e atanh(e sin phi), the conformal
    latitude chi = gd(psi) = asin(tanh(psi)), and the spherical stereographic formula on the conformal sphere.  Only the spelling
    of the conformal latitude differs from py4cast_amd.datasets.stereographic_forward; the final stereographic expression is
    the same.  The pin therefore guards against a slip in either spelling, not against a wrong choice of ellipsoid, scale factor
    or centre (tests/golden/README.md)."""
    a, f = 6378137.0, 1 / 298.257223563
    e = np.sqrt(f * (2 - f))

    def chi_of(phi):
        s = np.sin(phi)
        return np.arcsin(np.tanh(np.arctanh(s) - e * np.arctanh(e * s)))

    phi1 = np.radians(45.0)
    chi1 = chi_of(phi1)
    radius = a * np.cos(phi1) / np.sqrt(1 - (e * np.sin(phi1)) ** 2) / np.cos(chi1)
    out = {}
    for corner, (lon, lat) in R_DOMAIN.items():
        chi, lam = chi_of(np.radians(lat)), np.radians(lon)
        k = 2 / (1 + np.sin(chi1) * np.sin(chi) + np.cos(chi1) * np.cos(chi) * np.cos(lam))
        out[corner] = {"lon": lon, "lat": lat, "x": float(radius * k * np.cos(chi) * np.sin(lam)),
                       "y": float(radius * k * (np.cos(chi1) * np.sin(chi) - np.sin(chi1) * np.cos(chi) * np.cos(lam)))}
    return out


R_DOMAIN = None

if __name__ == "__main__":
    tmp = Path(tempfile.mkdtemp(prefix="golden_datasets_"))
    R = install(tmp)
    g = np.random.default_rng(2024)
    confs = {}

    # ---------------------------------------------------------------- periods
    obs = R.access.Period(name="train", start=20230101, end=20230103, obs_step=3600, obs_step_btw_t0=10800)
    ref = R.access.Period(name="train", start=20210615, end=20210616, refcst_daily_runs=[10800, 75600], refcst_leadtime_start_in_sec=0,
                          refcst_leadtime_end_in_sec=172800, refcst_leadtime_step_in_sec=10800)
    pairs = lambda p: [[iso(t0), int(lt.total_seconds())] for t0, lt in p.available_t0_and_leadtimes]  # noqa: E731
    write_json("datasets_periods.json", {
        "obs": {"kwargs": dict(start=20230101, end=20230103, obs_step=3600, obs_step_btw_t0=10800), "pairs": pairs(obs),
                "forecast_step": obs.forecast_step.total_seconds()},
        "refcst": {"kwargs": dict(start=20210615, end=20210616, refcst_daily_runs=[10800, 75600], refcst_leadtime_start_in_sec=0,
                                  refcst_leadtime_end_in_sec=172800, refcst_leadtime_step_in_sec=10800), "pairs": pairs(ref),
                   "forecast_step": ref.forecast_step.total_seconds()}})

    # ---------------------------------------------------------------- statics
    lat, lon = np.linspace(51.0, 49.0, 5), np.linspace(-3.0, 6.0, 7)
    geo = g.standard_normal((5, 7)) * 300 + 400
    st = {"lat": lat, "lon": lon, "geopotential": geo}
    for key, border, gp in (("border0", 0, geo), ("border1", 1, geo), ("constant", 1, np.full((5, 7), 7.5))):
        grid = R.access.Grid(name="g", load_grid_info_func=lambda n, gp=gp: R.access.GridConfig((5, 7), lat, lon, gp, None), border_size=border)
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            nt = R.access.grid_static_features(grid, [])
        st[key] = nt.tensor.numpy()
        st[f"{key}_names"] = np.array(nt.feature_names)
        st[f"{key}_limits"] = np.array(grid.grid_limits)
    np.savez_compressed(os.path.join(HERE, "datasets_statics.npz"), **st)
    print("datasets_statics.npz:", os.path.getsize(os.path.join(HERE, "datasets_statics.npz")), "bytes")

    # ---------------------------------------------------------------- dummy: the observation enumerations and Sample.load
    samples = {}
    dummy_conf = {"grid": {"name": "dummygrid", "border_size": 0, "subdomain": [0, 64, 0, 64], "proj_name": "PlateCarree", "projection_kwargs": {}},
                  "params": {"dummy_parameter": {"kind": "input_output", "levels": [500]}},
                  "periods": {p: dict(start=20230101, end=20230103, obs_step=3600, obs_step_btw_t0=10800) for p in ("train", "valid", "test")},
                  "settings": {"file_format": "npy", "standardize": True}}
    confs["dummy"] = dummy_conf
    tr11, va11, _ = R.base.DatasetABC.from_dict(R.dummy.DummyAccessor, "dummy", dummy_conf, 1, 1, 1)
    tr23, va23, _ = R.base.DatasetABC.from_dict(R.dummy.DummyAccessor, "dummy", dummy_conf, 2, 3, 3)
    samples["obs_1_1"], samples["obs_2_3"] = stamps_of(tr11), stamps_of(tr23)
    _ = tr11[0]     # the reference writes dummy_data.npy on first use, as long as this first sample
    root = Path(os.environ["PY4CAST_ROOTDIR"]) / "cache" / "dummy_dummygrid"
    load_fixture(R, "dummy", tr11, {"dummy_dummygrid/dummy_data.npy": np.load(root / "dummy_data.npy")},
                 {"dummy_parameter_500_isobaricInhPa": {"mean": 0.0, "std": 1.0, "max": 3.0, "min": -3.0}},
                 {"dummy_parameter_500_isobaricInhPa": {"mean": 0.0, "std": 1.42}}, 3, {"steps": [1, 1, 1]})

    # ---------------------------------------------------------------- poesy
    with open(Path(mg.REF) / "py4cast/datasets/poesy/metadata.yaml") as f:
        full = yaml.safe_load(f)
    pmeta = {"TERMS": full["TERMS"], "WEATHER_PARAMS": {k: {kk: vv for kk, vv in full["WEATHER_PARAMS"][k].items() if kk != "extent"}
                                                        for k in ("t2m", "tirf")}}
    proot = tmp / "poesy"
    proot.mkdir()
    R.poesy.SCRATCH_PATH, R.poesy.METADATA = proot, pmeta
    H, W = 10, 9
    oro = (g.standard_normal((H, W)) * 200).astype(np.float32)
    latlon = np.stack([np.repeat(np.linspace(-2.0, 6.0, W)[None], H, 0), np.repeat(np.linspace(50.0, 44.0, H)[:, None], W, 1)]).astype(np.float64)
    pfiles = {R.poesy.OROGRAPHY_FNAME: oro, R.poesy.LATLON_FNAME: latlon}
    np.save(proot / R.poesy.OROGRAPHY_FNAME, oro)
    np.save(proot / R.poesy.LATLON_FNAME, latlon)
    poesy_conf = {"grid": {"name": "EURW1S40_tiny", "border_size": 1, "subdomain": [1, 9, 2, 9], "proj_name": "LambertConformal",
                           "projection_kwargs": {"central_longitude": 2, "central_latitude": 46.7}},
                  "params": {"t2m": {"kind": "input_output", "levels": [2]}, "tirf": {"kind": "input_output", "levels": [0]}},
                  "periods": {p: dict(start=20210615, end=20210616, refcst_daily_runs=[10800, 75600], refcst_leadtime_start_in_sec=0,
                                      refcst_leadtime_end_in_sec=172800, refcst_leadtime_step_in_sec=10800) for p in ("train", "valid", "test")},
                  "settings": {"file_format": "npy", "standardize": True}, "members": [0, 1]}
    confs["poesy"], confs["poesy_metadata"] = poesy_conf, pmeta
    runs = [dt.datetime(2021, 6, d) + dt.timedelta(seconds=s) for d in (15, 16) for s in (10800, 75600)]
    touched = []
    for ri, run in enumerate(runs):
        for pname, fname in (("t2m", "t2m"), ("tirf", "rrdecum")):
            rel = f"{run.strftime('%Y-%m-%dT%H:%M:%SZ')}_{fname}_lt1-45_crop.npy"
            if ri == 2 and pname == "tirf":
                continue                               # a missing file: every sample of this run is dropped
            if ri == 0:                                # the run whose samples are loaded; the others only have to exist
                arr = (g.standard_normal((H, W, 45, 2)) * (5 if pname == "t2m" else 1) + (280 if pname == "t2m" else 0)).astype(np.float32)
                np.save(proot / rel, arr)
                pfiles[rel] = arr
            else:
                np.save(proot / rel, np.zeros((1, 1, 45, 2), np.float32))
                touched.append(rel)
    pstats = {"t2m_2_heightAboveGround": {"mean": 280.5, "std": 4.5, "min": 250.0, "max": 310.0},
              "tirf_0_surface": {"mean": 0.1, "std": 1.1, "min": -5.0, "max": 5.0}}
    pdiff = {k: {"mean": 0.0, "std": 1.3} for k in pstats}
    cache = Path(os.environ["PY4CAST_ROOTDIR"]) / "cache" / "poesy_EURW1S40_tiny"
    save_stats(cache / "parameters_stats.pt", pstats)
    save_stats(cache / "diff_stats.pt", pdiff)
    ptr, _, _ = R.base.DatasetABC.from_dict(R.poesy.PoesyAccessor, "poesy", poesy_conf, 2, 2, 2)
    samples["poesy_2_2"] = stamps_of(ptr)
    load_fixture(R, "poesy", ptr, pfiles, pstats, pdiff, 4, {"steps": [2, 2, 2], "touch": touched})

    # ---------------------------------------------------------------- rainfall
    R_DOMAIN = dict(R.rainfall.DOMAIN)
    corners = rainfall_corners()
    write_json("datasets_rainfall_corners.json", {"source": "closed form (see make_golden_datasets.rainfall_corners): cartopy is absent and "
                                                            "its stub gives no numbers", "central_latitude": 45, "corners": corners})
    # domain_to_extent needs cartopy: the reference's own function body is run with the pinned corners standing for transform_point
    R.rainfall.Stereographic = lambda central_latitude: types.SimpleNamespace(
        transform_point=lambda lon, lat, src: next((c["x"], c["y"]) for c in corners.values() if (c["lon"], c["lat"]) == (lon, lat)))
    R.rainfall.PlateCarree = lambda: None
    rroot = tmp / "rain"
    R.rainfall.SCRATCH_PATH = rroot
    (rroot / "cache").mkdir(parents=True)
    rain_conf = {"grid": {"name": "rainfallgrid", "border_size": 0, "subdomain": [0, 16, 0, 16], "proj_name": "Stereographic",
                          "projection_kwargs": {"central_latitude": 45}},
                 "params": {"precip": {"levels": [0], "typeOfLevel": "surface", "kind": "input_output"}},
                 "periods": {p: dict(start=20240101, end=20240101, obs_step=300, obs_step_btw_t0=10800) for p in ("train", "valid", "test")},
                 "settings": {"standardize": True, "file_format": "npz"}}
    confs["rainfall"] = rain_conf
    rfiles, compressed = {}, []
    t0s = [dt.datetime(2024, 1, 1) + k * dt.timedelta(seconds=10800) for k in range(8)]
    for ti, t0 in enumerate(t0s):
        for d in range(-1, 4):
            date = t0 + d * dt.timedelta(seconds=300)
            if ti == 2 and d == 1:
                continue                               # a missing file: exactly the third sample is dropped
            rel = f"Hexagone/{date.year}/{date.strftime('%Y%m%d%H%M')}.npz"
            arr = np.maximum(g.gamma(0.3, 400.0, (16, 16)), 0).astype(np.int16)
            arr[g.random((16, 16)) < 0.2] = -1        # outside of the radar field
            arr[0, 0], arr[15, 15] = 32767, -32768
            (rroot / rel).parent.mkdir(parents=True, exist_ok=True)
            if (ti + d) % 2:
                np.savez_compressed(rroot / rel, arr)
                compressed.append(rel)
            else:
                np.savez(rroot / rel, arr)
            rfiles[rel] = arr
    rstats = {"precip": {"mean": 0.7, "std": 2.3, "min": 0.0, "max": 3932.0}}
    rdiff = {"precip": {"mean": 0.0, "std": 1.9}}
    save_stats(rroot / "cache" / "parameters_stats.pt", rstats)
    save_stats(rroot / "cache" / "diff_stats.pt", rdiff)
    rtr, rva, _ = R.base.DatasetABC.from_dict(R.rainfall.RainfallAccessor, "rainfall", rain_conf, 2, 1, 3)
    samples["rainfall_2_3"] = stamps_of(rva)
    load_fixture(R, "rainfall", rva, rfiles, rstats, rdiff, 3, {"steps": [2, 1, 3], "compressed": compressed, "period": "valid"})

    # ---------------------------------------------------------------- titan, file_format npy
    with open(Path(mg.REF) / "py4cast/datasets/titan/metadata.yaml") as f:
        full = yaml.safe_load(f)
    keep = ("grib", "grid", "long_name", "param", "type_level", "unit", "name")
    tmeta = {"GRIDS": {"PAAROME_1S100": {"size": [12, 9], "extent": full["GRIDS"]["PAAROME_1S100"]["extent"]}},
             "WEATHER_PARAMS": {k: {kk: full["WEATHER_PARAMS"][k].get(kk) for kk in keep} for k in ("aro_t2m", "aro_t", "aro_r2")}}
    R.titan.METADATA = tmeta
    troot = Path(os.environ["PY4CAST_TITAN_PATH"])
    troot.mkdir(parents=True)
    gr.NI, gr.NJ = 9, 12
    height = (g.random((12, 9)) * 900).astype(np.float32)
    s4 = gr.section4(3, 6, 1, None)
    conf_grib = gr.message(0, gr.section1(dt.datetime(2020, 1, 1)), gr.section3(False, ni=9, nj=12), s4, height.reshape(-1), 1, 16)
    from py4cast_amd import grib2   # the package's own decoder says what the file holds: the reference's xarray is absent

    msg = grib2.parse_messages(conf_grib)[0]
    _, _, glat, glon, _ = grib2.grid_of(msg)
    gh = np.ma.filled(grib2.decode(msg)[0], np.nan)
    R.titan.xr.open_dataset = lambda path: types.SimpleNamespace(latitude=types.SimpleNamespace(values=glat), longitude=types.SimpleNamespace(values=glon),
                                                                 h=types.SimpleNamespace(values=gh))
    titan_conf = {"grid": {"name": "PAAROME_1S100", "border_size": 2, "subdomain": [0, 12, 0, 9], "proj_name": "PlateCarree", "projection_kwargs": {}},
                  "params": {"aro_t2m": {"levels": [2], "kind": "input_output"}, "aro_r2": {"levels": [2], "kind": "input"},
                             "aro_t": {"levels": [850, 500], "kind": "input_output"}},
                  "periods": {p: dict(start=20230301, end=20230301, obs_step=3600, obs_step_btw_t0=21600) for p in ("train", "valid", "test")},
                  "settings": {"standardize": True, "file_format": "npy"}}
    confs["titan"], confs["titan_metadata"] = titan_conf, tmeta
    sub = "subdatasets/titan_PAAROME_1S100_0-12-0-9"
    tfiles = {"conf_PAAROME_1S100.grib": np.frombuffer(conf_grib, dtype=np.uint8)}
    names = {"aro_t2m_2m": (np.float32, 280, 8), "aro_r2_2m": (np.float64, 70, 20), "aro_t_850hpa": (np.float32, 270, 6),
             "aro_t_500hpa": (np.float32, 250, 5)}
    for k in range(4):
        for d in range(0, 3):
            date = dt.datetime(2023, 3, 1) + dt.timedelta(hours=6 * k + d)
            if k == 3 and d == 2:
                continue                               # a missing date: the last sample is dropped
            for n, (dtp, m, s) in names.items():
                rel = f"{sub}/data/{date.strftime('%Y-%m-%d_%Hh%M')}/{n}.npy"
                arr = (g.standard_normal((12, 9)) * s + m).astype(dtp)
                (troot / rel).parent.mkdir(parents=True, exist_ok=True)
                np.save(troot / rel, arr)
                tfiles[rel] = arr
    tstats = {n: {"mean": float(m), "std": float(s), "min": float(m - 4 * s), "max": float(m + 4 * s)} for n, (_, m, s) in names.items()}
    tdiff = {n: {"mean": 0.0, "std": 1.2} for n in names}
    save_stats(troot / sub / "parameters_stats.pt", tstats)
    save_stats(troot / sub / "diff_stats.pt", tdiff)
    ttr, _, _ = R.base.DatasetABC.from_dict(R.titan.TitanAccessor, "titan", titan_conf, 1, 2, 2)
    samples["titan_1_2"] = stamps_of(ttr)
    load_fixture(R, "titan", ttr, tfiles, tstats, tdiff, 3, {"steps": [1, 2, 2]})

    write_json("datasets_samples.json", samples)
    write_json("datasets_confs.json", confs)
