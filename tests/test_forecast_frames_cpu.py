"""
The forecast frames without a GPU: the closed form of tests/forecast_frames_closed_form.py against matplotlib itself on every data
case of the GPU test, the share of its band, the display table against the values of the reference (tests/golden/
forecast_display.json), the output paths, the GIF round trip through PIL, the launch arithmetic of csrc/forecast_frames.hip from its
query functions, and the sample bookkeeping of predict_step on a stub module.
"""
import json
import os
import sys
import types
import warnings
from datetime import datetime
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forecast_frames_closed_form as cf  # noqa: E402

GOLDEN = Path(__file__).parent / "golden" / "forecast_display.json"
CMAPS = ["Spectral_r", "plasma", "RdBu", "Spectral"]      # feature k of a case is looked up in colour table k % 4


@pytest.fixture(scope="module")
def cases():
    return {name: (c, cf.expected(c)) for name, c in cf.all_cases().items()}


@pytest.mark.parametrize("name", sorted(cf.SHAPES) + ["loop_dense", "loop_gather"])
def test_the_closed_form_equals_matplotlib_outside_the_band(name, cases):
    """frame by frame as the reference draws it: the floor as np.where(data < floor, nan, data), imshow's masked_invalid, Normalize
    with the given range or None (auto-scaled over what is not masked), the colormap resampled to 255 colours; the palette entry of
    the closed form's index is matplotlib's colour, and its bad pixels are matplotlib's transparent ones"""
    from matplotlib import colormaps
    from matplotlib.colors import Normalize

    from py4cast_amd.outputs import palette_for

    c, ((v, bad, vrange), want) = cases[name]
    H, W = c["H"], c["W"]
    n, T, K, N = v.shape
    features = list(range(K)) if c["features"] is None else list(c["features"])
    share = float(want["band"].mean())
    print(f"forecast frames {name}: band share {share:.3e}")
    assert share <= 1e-2          # a condition on the data: the GPU test cannot hide a failure inside the band
    palettes = {m: palette_for(m) for m in CMAPS}
    drawn = 0
    for k, f in enumerate(features):
        off, flo, lo, hi = c["display"][f]
        cmap = colormaps[CMAPS[k % 4]].resampled(255)
        for s in range(n):
            for t in range(T):
                data = v[s, t, k].double().numpy().reshape(H, W)      # un-normalised, offset added: what the reference hands plot_frame
                if flo is not None:
                    with np.errstate(invalid="ignore"):
                        data = np.where(data < flo, np.nan, data)
                masked = np.ma.masked_invalid(data)
                index = want["index"][s, t, k]
                if masked.mask.all():
                    assert (index == cf.BAD).all() and torch.isnan(vrange[s, t, k]).all()
                    continue
                norm = Normalize(vmin=lo, vmax=hi)
                rgba = cmap(norm(masked), bytes=True)[::-1]              # origin="lower"
                assert (float(norm.vmin), float(norm.vmax)) == (float(vrange[s, t, k, 0]), float(vrange[s, t, k, 1]))
                assert np.array_equal(rgba[..., 3] == 0, index == cf.BAD)
                keep = ~want["band"][s, t, k] & (index != cf.BAD)
                assert np.array_equal(palettes[CMAPS[k % 4]][index][keep], rgba[..., :3][keep]), (name, s, t, k)
                drawn += 1
    assert drawn >= n * T * K - 2


def test_display_for_equals_the_reference_values():
    from py4cast_amd.outputs import DEFAULT_DISPLAY, FeatureDisplay, display_for

    golden = json.loads(GOLDEN.read_text())
    names = [f"aro_{p}_2m" for p in golden["params"]] + [f"arp_{p}_10m" for p in golden["params"]]
    names += ["aro_z_500hpa", "orography", "aro_prmsl_0hpa"]          # an unknown parameter, a one-token name, another unknown one
    rows = display_for(names)
    assert len(rows) == len(names)
    for name, row in zip(names, rows):
        tokens = name.split("_")
        want = golden["params"].get(tokens[1], golden["default"]) if len(tokens) > 1 else golden["default"]
        assert (row.cmap, row.vmin, row.vmax, row.floor) == (want["cmap"], want["vmin"], want["vmax"], want["floor"]), name
        assert row.offset == golden["offsets"].get(name, 0.0), name
    assert rows[names.index("aro_t2m_2m")].offset == -273.15 and rows[names.index("arp_t2m_10m")].offset == 0.0
    assert rows[names.index("orography")] == DEFAULT_DISPLAY == FeatureDisplay("plasma")
    own = display_for(["aro_z_500hpa", "x_t2m"], table={"z": FeatureDisplay("viridis", 4900.0, 5900.0)}, offsets={"x_t2m": 1.0})
    assert own == [FeatureDisplay("viridis", 4900.0, 5900.0), FeatureDisplay("plasma", offset=1.0)]


TITAN = {   # the values of the reference's config/IO/titan_grib_settings.json, directories aside
    "template_grib": "../template/grid.arome-oper.eurw1s40+0001:00.grib", "path_to_runtime": "dataset_{}/{}",
    "output_kwargs": ["titan_1s40"], "grib_fmt": "mb{}/forecast/grid.emul_aro_ai_ech_{}.grib", "grib_identifiers": ["member", "leadtime"],
    "gif_fmt": "{}_feature_{}.gif", "gif_identifiers": ["runtime", "feature"],
}
POESY = {   # config/IO/poesy_grib_settings.json: the older layout, which the reference's OutputSavingSettings(**json) refuses as well
    "template_grib": "../template/grid.arome-oper.eurw1s40+0001:00.grib", "directory": "/scratch/shared/py4cast/gribs_writing/todel/",
    "output_kwargs": ["poesy_eurw1s40"], "sample_identifiers": ["runtime", "member", "leadtime"],
    "output_fmt": "dataset_{}/{}/mb{}/forecast/grid.emul_aro_ai_ech_{}.grib",
}


def _settings(tmp_path, **values):
    from py4cast_amd.outputs import OutputSavingSettings

    path = tmp_path / "io.json"
    path.write_text(json.dumps(dict(values, dir_grib=str(tmp_path / "gribs"), dir_gif=str(tmp_path / "gifs"))))
    return OutputSavingSettings.from_json(path)


def test_gif_paths_of_the_reference_layouts(tmp_path):
    from py4cast_amd.outputs import OutputSavingSettings

    titan = _settings(tmp_path, **TITAN)
    path = titan.get_gif_path("2023010112", "aro_t2m_2m")
    assert path == tmp_path / "gifs" / "dataset_titan_1s40" / "2023010112" / "2023010112_feature_aro_t2m_2m.gif"
    assert path.parent.is_dir() and not path.exists()
    # the dataclass's defaults: no output_kwargs, the runtime alone
    plain = _settings(tmp_path, template_grib="t.grib", path_to_runtime="{}")
    assert plain.gif_fmt == "{}_feature_{}.gif" and tuple(plain.gif_identifiers) == ("runtime", "feature") and tuple(plain.output_kwargs) == ()
    assert plain.get_gif_path("sample000003", "aro_tp_0m") == tmp_path / "gifs" / "sample000003" / "sample000003_feature_aro_tp_0m.gif"
    swapped = _settings(tmp_path, **dict(TITAN, gif_fmt="{}/{}.gif", gif_identifiers=["feature", "runtime"]))
    assert swapped.get_gif_path("2023010112", "aro_r2_2m") == tmp_path / "gifs" / "dataset_titan_1s40" / "2023010112" / "aro_r2_2m" / "2023010112.gif"
    with pytest.raises(TypeError):
        path = tmp_path / "poesy.json"
        path.write_text(json.dumps(POESY))
        OutputSavingSettings.from_json(path)
    with pytest.raises(ValueError, match=r"\{\}_feature_\{\}\.gif has 2 placeholders.*but 1 identifiers"):
        _settings(tmp_path, **dict(TITAN, gif_identifiers=["runtime"])).get_gif_path("r", "f")
    with pytest.raises(ValueError, match=r"dataset_\{\}/\{\} has 1 placeholders.*but 2 identifiers"):
        _settings(tmp_path, **dict(TITAN, output_kwargs=["a", "b"])).get_gif_path("r", "f")


def test_gif_round_trip_of_three_different_frames(tmp_path):
    from PIL import Image

    from py4cast_amd.outputs import palette_for, save_palette_gif

    g = np.random.default_rng(3)
    H, W = 33, 47
    frames = g.integers(0, 256, size=(3, H, W)).astype(np.uint8)
    frames[1, 4:9, :] = 255                 # a band of bad pixels; frame 2 keeps large parts of frame 1 (the encoder may crop to the change)
    frames[2, :20] = frames[1, :20]
    for name, palette in (("synthetic", cf.synthetic_palette()), ("Spectral_r", palette_for("Spectral_r"))):
        path = tmp_path / f"{name}.gif"
        save_palette_gif(path, frames, palette)
        with Image.open(path) as gif:
            assert gif.n_frames == 3 and gif.size == (W, H) and gif.info.get("loop") == 0
            for t in range(3):
                gif.seek(t)
                assert gif.info["duration"] == 500
                assert np.array_equal(np.asarray(gif.convert("RGB")), palette[frames[t]]), (name, t)
    white = palette_for("plasma")
    assert white.shape == (256, 3) and white.dtype == np.uint8 and (white[255] == 255).all()


def test_launch_arithmetic_from_the_query_functions():
    """what tests/test_forecast_frames_gpu.py sizes its second-trip case from"""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    handle = L.lib()
    tile, cap = handle.p4c_forecast_tile(), handle.p4c_forecast_max_blocks()
    assert (tile, cap) == (ops.FORECAST_TILE, ops.FORECAST_MAX_BLOCKS)
    assert (handle.p4c_forecast_max_features(), handle.p4c_forecast_max_samples()) == (ops.FORECAST_MAX_FEATURES, ops.FORECAST_MAX_SAMPLES)
    for n, T, N, K in [(1, 1, 1, 1), (2, 3, 512 * 512, 60), (2, 3, 512 * 640, 21), (2, 2, 33 * 997, 3), (256, 255, 5, 2), (3, 1, tile * cap, 7)]:
        tiles = -(-N // tile)
        blocks = min(tiles, max(1, cap // (n * T)))        # workgroups of one (sample, lead time); they stride over its tiles
        assert handle.p4c_forecast_frames_workspace_bytes(n, T, N, K) == n * T * blocks * K * 2 * 4, (n, T, N, K)
    assert handle.p4c_forecast_frames_workspace_bytes(0, 1, 1, 1) == 0
    # the rule of the two forms: whole points through LDS when at least half of at most 64 features are drawn
    for K, F, dense in [(60, 60, True), (21, 21, True), (64, 64, True), (65, 65, False), (3, 21, False), (11, 21, True), (10, 21, False),
                        (4, 60, False), (2, 4, True), (3, 8, False)]:
        assert bool(handle.p4c_forecast_frames_dense(K, F)) == dense, (K, F)


class _Writer:
    def __init__(self):
        self.calls = []

    def submit(self, preds, std, mean, runtimes, accepted):
        self.calls.append((list(runtimes), list(accepted)))


def _stub(tmp_path, sample_list=None, datamodule=None, **attrs):
    from py4cast_amd.lightning import AutoRegressiveLightning as ARL

    class Stub:
        forecast_samples, _datamodule, _write_forecast_outputs = ARL.forecast_samples, ARL._datamodule, ARL._write_forecast_outputs

    io = tmp_path / "io.json"
    io.write_text(json.dumps(dict(TITAN, dir_grib=str(tmp_path / "gribs"), dir_gif=str(tmp_path / "gifs"))))
    stub = Stub()
    stub.io_conf = io
    stub.infer_ds = None if sample_list is None else types.SimpleNamespace(sample_list=sample_list)
    stub.trainer = types.SimpleNamespace(datamodule=datamodule) if datamodule is not None else types.SimpleNamespace()
    stub.forecast_writer = _Writer()
    for k, v in attrs.items():
        setattr(stub, k, v)
    return stub


def test_accepted_samples_and_runtimes_of_predict_step(tmp_path):
    dates = [datetime(2023, 1, 1, h) for h in (0, 3, 6, 12, 18, 21)]
    samples = [types.SimpleNamespace(timestamps=types.SimpleNamespace(datetime=d)) for d in dates]
    preds = types.SimpleNamespace(tensor=torch.zeros(2, 1, 1, 1, 1))
    dm = types.SimpleNamespace(list_run_hour=[0, 12, 18], save_gifs=True, save_gribs=False)
    stub = _stub(tmp_path, samples, dm)
    assert stub.forecast_samples(0, 2) == (["2023010100", "2023010103"], [True, False])
    assert stub.forecast_samples(1, 2) == (["2023010106", "2023010112"], [False, True])
    assert stub.forecast_samples(2, 2) == (["2023010118", "2023010121"], [True, False])
    stub._write_forecast_outputs(1, preds, None, None)
    assert stub.forecast_writer.calls == [(["2023010106", "2023010112"], [False, True])]
    settings = stub._output_settings
    stub._write_forecast_outputs(2, preds, None, None)
    assert stub._output_settings is settings and len(stub.forecast_writer.calls) == 2        # the settings are read once
    # no sample of the batch is accepted: nothing is submitted
    none = _stub(tmp_path, samples, types.SimpleNamespace(list_run_hour=[1], save_gifs=True, save_gribs=True))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        none._write_forecast_outputs(0, preds, None, None)
    assert none.forecast_writer.calls == []
    # save_gifs off: nothing; save_gribs: one warning, once
    off = _stub(tmp_path, samples, types.SimpleNamespace(list_run_hour=[0, 3], save_gifs=False, save_gribs=True))
    with pytest.warns(UserWarning, match="epygram"):
        off._write_forecast_outputs(0, preds, None, None)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        off._write_forecast_outputs(0, preds, None, None)
    assert off.forecast_writer.calls == []
    # no datamodule, no sample list: every sample, named by its index; the module's own save_gifs
    bare = _stub(tmp_path)
    assert bare.forecast_samples(3, 2) == (["sample000006", "sample000007"], [True, True])
    bare._write_forecast_outputs(3, preds, None, None)
    assert bare.forecast_writer.calls == [(["sample000006", "sample000007"], [True, True])]
    quiet = _stub(tmp_path, save_gifs=False)
    quiet._write_forecast_outputs(0, preds, None, None)
    assert quiet.forecast_writer.calls == []
    # a sample list without a datamodule: dated names, all accepted
    dated = _stub(tmp_path, samples)
    assert dated.forecast_samples(0, 2) == (["2023010100", "2023010103"], [True, True])


def test_the_writer_names_the_missing_package(monkeypatch):
    import builtins

    from py4cast_amd.outputs import ForecastGifWriter, OutputSavingSettings

    settings = OutputSavingSettings("t", "g", "d", "{}")
    real = builtins.__import__
    for package in ("PIL", "matplotlib"):
        def fake(name, *a, _package=package, **k):
            if name == _package:
                raise ImportError(name)
            return real(name, *a, **k)

        monkeypatch.setattr(builtins, "__import__", fake)
        with pytest.raises(RuntimeError, match=package):
            ForecastGifWriter(settings, torch.device("cuda", 0))
        monkeypatch.setattr(builtins, "__import__", real)
    with pytest.raises(RuntimeError, match="GPU"):
        ForecastGifWriter(settings, torch.device("cpu"))
