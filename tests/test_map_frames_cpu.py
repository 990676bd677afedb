"""
The host side of the native prediction-map observers, without a GPU: the closed form the GPU tests compare with (against
matplotlib's own colour mapping, and the share of pixels its band leaves out for the seeds the GPU tests use), the ABI, the
argument checks, the bookkeeping of MapPlot, the figures / GIF composed from finished frames, and the Lightning lists.
"""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_frames_closed_form as cf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _have_matplotlib():
    try:
        import matplotlib  # noqa: F401

        return True
    except Exception:
        return False


class Experiment:
    def __init__(self):
        self.figures = []

    def add_figure(self, name, fig, step):
        self.figures.append((name, fig, int(step)))


# ------------------------------------------------------------------------------------------------ the closed form
def _normal_planes(seed, n, T, K, H, W):
    """as test_map_frames_gpu._render_case(special=False)"""
    g = torch.Generator().manual_seed(seed)
    planes = torch.randn(n, T, K, 2, H * W, generator=g) * 3 + 1
    flat = planes[:, :, :, 0].permute(0, 2, 1, 3).reshape(n, K, -1)
    return planes, torch.stack([flat.amin(dim=-1), flat.amax(dim=-1)], dim=-1)


@pytest.mark.parametrize("seed,shape", [(1, (2, 2, 3, 13, 37)), (2, (2, 2, 3, 64, 64)), (4, (1, 2, 4, 128, 256)), (6, (1, 1, 1, 13, 37))])
def test_band_share_of_the_gpu_tests_seeds(seed, shape):
    """the closed form alone: the pixels within 2^-13 of an index boundary stay under 1e-3 of the frame for every seed used"""
    n, T, K, H, W = shape
    planes, vrange = _normal_planes(seed, n, T, K, H, W)
    want = cf.render(planes.numpy(), vrange.numpy(), cf.synthetic_lut(), cf.border_interior(H, W, 2), H, W)
    assert want["band"].mean() <= 1e-3
    assert cf.compare(want["frames"], want) == want["band"].mean()


def test_closed_form_layout():
    H, W = 3, 4
    planes = torch.zeros(1, 1, 1, 2, H * W)
    planes[0, 0, 0, 0] = torch.arange(12.0)            # target: 0 .. 11, grid row 0 first
    planes[0, 0, 0, 1] = torch.tensor([-5.0] * 6 + [20.0] * 5 + [float("nan")])
    vrange = torch.tensor([[[0.0, 11.0]]])
    lut = cf.synthetic_lut()
    out = cf.render(planes.numpy(), vrange.numpy(), lut, np.ones((H, W), dtype=np.float32), H, W)
    f = out["frames"][0, 0, 0]
    assert f.shape == (H, 2 * W + cf.GAP, 3) and (f[:, W:W + cf.GAP] == 255).all()
    assert (f[H - 1, 0] == lut[0]).all() and (f[0, W - 1] == lut[255]).all()         # origin lower; the maximum takes the last entry
    assert (f[H - 1, 1] == lut[int(256 * 1 / 11)]).all()
    assert (f[H - 1, W + cf.GAP] == lut[0]).all() and (f[0, W + cf.GAP] == lut[255]).all()   # below / above the range
    assert (f[0, 2 * W + cf.GAP - 1] == 255).all()                                   # NaN
    faded = cf.render(planes.numpy(), vrange.numpy(), lut, np.zeros((H, W), dtype=np.float32), H, W)["frames"][0, 0, 0]
    assert (faded[H - 1, 0] == np.floor(0.7 * lut[0].astype(np.float64) + 0.3 * 255 + 0.5)).all()


@pytest.mark.skipif(not _have_matplotlib(), reason="matplotlib's own colour mapping is the reference here")
def test_closed_form_equals_matplotlib_on_interior_pixels():
    from matplotlib import colormaps
    from matplotlib.colors import Normalize

    from py4cast_amd.observers import plasma_table

    H, W = 64, 64
    planes, vrange = _normal_planes(2, 2, 2, 3, H, W)
    want = cf.render(planes.numpy(), vrange.numpy(), plasma_table(), cf.border_interior(H, W, 2), H, W)
    keep = ~want["band"] & want["exact"]
    for s in range(2):
        for k in range(3):
            norm = Normalize(vmin=float(vrange[s, k, 0]), vmax=float(vrange[s, k, 1]))
            for panel, c0 in ((0, 0), (1, W + cf.GAP)):
                rgb = colormaps["plasma"](norm(planes[s, 1, k, panel].numpy().reshape(H, W)[::-1]), bytes=True)[..., :3]
                m = keep[s, 1, k, :, c0:c0 + W]
                assert np.array_equal(want["frames"][s, 1, k, :, c0:c0 + W][m], rgb[m])


def test_planes_restatement_is_the_references_expression():
    g = torch.Generator().manual_seed(0)
    pred, target = torch.randn(2, 2, 3, 4, 5, generator=g), torch.randn(2, 2, 3, 4, 5, generator=g)
    mask = torch.rand(2, 2, 3, 4, 5, generator=g) > 0.5
    std, mean = torch.rand(5, generator=g) + 0.5, torch.randn(5, generator=g)
    planes, vrange = cf.planes(pred, target, mask, std, mean, (3, 1), 1)
    p, t = (pred * mask) * std + mean, target * std + mean                            # plots.py:271, 299-300
    assert torch.equal(planes[0, 1, 0, 1].reshape(3, 4), p[0, 1, :, :, 3]) and torch.equal(planes[0, 0, 1, 0].reshape(3, 4), t[0, 0, :, :, 1])
    assert torch.equal(vrange[0, :, 0], t[0].flatten(0, 2).min(dim=0)[0][[3, 1]])    # plots.py:311
    assert torch.equal(vrange[0, :, 1], t[0].flatten(0, 2).max(dim=0)[0][[3, 1]])


# ------------------------------------------------------------------------------------------------ ABI and argument checks
def test_abi_gains_the_map_functions():
    from py4cast_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "py4cast_hip.h")).read()
    for name in ("p4c_map_planes", "p4c_map_render", "p4c_map_planes_workspace_bytes", "p4c_map_tile", "p4c_map_max_blocks", "p4c_map_gap",
                 "p4c_map_render_pixels", "p4c_map_render_max_blocks"):
        assert name in _lib.all_symbols() and re.search(rf"\b{name}\(", header)
    assert len(_lib.SIGNATURES["p4c_map_planes"]) == 20 and len(_lib.SIGNATURES["p4c_map_render"]) == 11
    source = open(os.path.join(ROOT, "py4cast_amd", "csrc", "map_frames.hip")).read()
    for c_name, value in (("MAP_TILE", ops.MAP_TILE), ("MAP_MAX_BLOCKS", ops.MAP_MAX_BLOCKS), ("MAP_MAX_FEATURES", ops.MAP_MAX_FEATURES),
                          ("MAP_GAP", ops.MAP_GAP), ("MAP_RENDER_PIXELS", ops.MAP_RENDER_PIXELS),
                          ("MAP_RENDER_MAX_BLOCKS", ops.MAP_RENDER_MAX_BLOCKS)):
        assert re.search(rf"constexpr int {c_name} = {value};", source), c_name
    assert ops.MAP_GAP == cf.GAP


def test_map_ops_have_no_cpu_path():
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    x = torch.zeros(1, 1, 2, 2, 3)
    with pytest.raises(L.P4CError, match="GPU only"):
        ops.map_planes(x, x, ops.MaskSpec(L.MASK_NONE), torch.ones(3), torch.zeros(3), (0,), 1)
    with pytest.raises(L.P4CError, match="GPU only"):
        ops.map_render(torch.zeros(1, 1, 1, 2, 4), torch.zeros(1, 1, 2), torch.zeros(256, 3, dtype=torch.uint8), torch.ones(4), 2, 2)


# ------------------------------------------------------------------------------------------------ bookkeeping
def _named(B=3, T=2, F=5, graph=False):
    from py4cast_amd.namedtensor import NamedTensor

    names = [f"v{i}" for i in range(F)]
    if graph:
        return NamedTensor(torch.zeros(B, T, 12, F), ["batch", "timestep", "ngrid", "features"], names)
    return NamedTensor(torch.zeros(B, T, 3, 4, F), ["batch", "timestep", "lat", "lon", "features"], names)


def test_sample_and_feature_selection():
    from py4cast_amd.observers import MapPlot, PredictionEpochPlot, PredictionTimestepPlot

    obj = types.SimpleNamespace(trainer=types.SimpleNamespace(is_global_zero=True), grid_shape=(3, 4))
    p = PredictionTimestepPlot(num_samples_to_plot=4, num_features_to_plot=2, prefix="Validation", save_path="/tmp/x")
    assert (p.num_samples_to_plot, p.num_features_to_plot, p.prefix, str(p.save_path), p.plotted_examples) == (4, 2, "Validation", "/tmp/x", 0)
    assert p.remaining(obj, 3) == 3
    p.plotted_examples = 3
    assert p.remaining(obj, 3) == 1
    p.plotted_examples = 4
    assert p.remaining(obj, 3) == 0
    p.plotted_examples = 0
    assert p.remaining(types.SimpleNamespace(trainer=types.SimpleNamespace(is_global_zero=False)), 3) == 0   # rank zero only
    assert p.feature_names(_named()) == ["v0", "v1"]
    assert PredictionEpochPlot(1).feature_names(_named()) == [f"v{i}" for i in range(5)]     # None: all of them
    assert PredictionEpochPlot(1, 0).feature_names(_named()) == [f"v{i}" for i in range(5)]  # plots.py:315-319 tests truth
    assert MapPlot.grid(obj, _named()) == (3, 4) and MapPlot.grid(obj, _named(graph=True)) == (3, 4)
    import inspect

    assert list(inspect.signature(PredictionTimestepPlot.__init__).parameters)[:5] == [
        "self", "num_samples_to_plot", "num_features_to_plot", "prefix", "save_path"]


def test_update_raises_on_cpu_tensors_and_skips_when_done():
    from py4cast_amd import _lib as L
    from py4cast_amd.base import Stats
    from py4cast_amd.observers import PredictionTimestepPlot

    named = _named()
    stats = Stats({n: {"std": torch.tensor(1.0), "mean": torch.tensor(0.0)} for n in named.feature_names})
    obj = types.SimpleNamespace(trainer=types.SimpleNamespace(is_global_zero=True), stats=stats)
    p = PredictionTimestepPlot(1, 2, lut=cf.synthetic_lut())
    with pytest.raises(L.P4CError, match="GPU only"):
        p.update(obj, None, named, named, None)
    p.plotted_examples = 1
    p.update(obj, None, named, named, None)          # nothing left to draw: the tensors are not touched
    assert p.plotted_examples == 1


def test_titles_with_and_without_dataset_attributes():
    from py4cast_amd.observers import PredictionEpochPlot, PredictionTimestepPlot

    full = types.SimpleNamespace(dataset_info=types.SimpleNamespace(units={"a": "K", "b": "m/s"}, pred_step=3), current_epoch=7)
    assert PredictionTimestepPlot(1).titles(full, ["a", "b"], 2) == ["a (K), t=2 (6 h)", "b (m/s), t=2 (6 h)"]       # plots.py:388-389
    assert PredictionEpochPlot(1).titles(full, ["a"], 4) == ["a (K), t=4 (12 h) - epoch 7"]                          # plots.py:453-454
    for bare in (types.SimpleNamespace(), types.SimpleNamespace(dataset_info=types.SimpleNamespace(units=None))):
        assert PredictionTimestepPlot(1).titles(bare, ["a"], 2) == ["a (), t=2 (2 h)"]
        assert PredictionEpochPlot(1).titles(bare, ["a"], 3) == ["a (), t=3 (3 h) - epoch 0"]


# ------------------------------------------------------------------------------------------------ figures and GIF from frames
def _frames(T, K, H, W, seed=0):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, size=(T, K, H, 2 * W + cf.GAP, 3)).astype(np.uint8), np.stack([np.zeros(K), np.ones(K)], axis=1).astype(np.float32)


def _obj(exp, **extra):
    return types.SimpleNamespace(trainer=types.SimpleNamespace(is_global_zero=True), logger=types.SimpleNamespace(experiment=exp),
                                 current_epoch=20, dataset_info=types.SimpleNamespace(units={"a": "K"}, pred_step=3), **extra)


@pytest.mark.skipif(not _have_matplotlib(), reason="figures need matplotlib")
def test_timestep_plot_writes_the_reference_names(tmp_path):
    from PIL import Image

    from py4cast_amd.observers import PredictionTimestepPlot

    T, K, H, W = 3, 2, 6, 9
    frames, vrange = _frames(T, K, H, W)
    vrange[1] = np.nan                              # a NaN range: the figure is still made, without a colour bar
    exp, logged = Experiment(), []
    mlflow = types.SimpleNamespace(version="run7", experiment=types.SimpleNamespace(
        log_figure=lambda run_id, figure, artifact_file: logged.append((run_id, artifact_file))))
    p = PredictionTimestepPlot(2, save_path=tmp_path)
    p.plotted_examples = 2
    p.plot_map(_obj(exp, mlflow_logger=mlflow), frames, vrange, ["a", "b"])
    d = tmp_path / "timestep_evol_per_param"
    assert sorted(f.name for f in d.iterdir()) == sorted([f"{v}_example_2_{t}.png" for v in "ab" for t in (1, 2, 3)] + ["a.gif", "b.gif"])
    assert [(f[0], f[2]) for f in exp.figures] == [(f"timestep_evol_per_param/{v}_example_2", t) for t in (1, 2, 3) for v in "ab"]
    assert logged[0] == ("run7", "figures/timestep_evol_per_param/a_example_2_1.png") and len(logged) == 6            # plots.py:409-415
    fig = exp.figures[0][1]
    assert fig._suptitle.get_text() == "a (K), t=1 (3 h)"
    assert [ax.get_title() for ax in fig.axes[:2]] == ["Ground Truth", "Prediction"] and len(fig.axes) == 3          # + the colour bar
    assert np.array_equal(np.asarray(fig.axes[0].images[0].get_array()), frames[0, 0, :, :W])
    assert np.array_equal(np.asarray(fig.axes[1].images[0].get_array()), frames[0, 0, :, W + cf.GAP:])
    assert len(exp.figures[1][1].axes) == 2                                                                           # NaN range
    with Image.open(d / "b.gif") as gif:
        assert gif.n_frames == T and gif.size == (2 * W + cf.GAP, H) and gif.info["duration"] == 250 and gif.info["loop"] == 0


@pytest.mark.skipif(not _have_matplotlib(), reason="figures need matplotlib")
def test_epoch_plot_writes_the_reference_names(tmp_path):
    from py4cast_amd.observers import PredictionEpochPlot

    frames, vrange = _frames(1, 2, 6, 9)
    exp = Experiment()
    p = PredictionEpochPlot(1, save_path=tmp_path)
    p.plotted_examples, p._max_step = 1, 4
    p.plot_map(_obj(exp), frames, vrange, ["a", "b"])
    assert sorted(f.name for f in (tmp_path / "epoch_evol_per_param").iterdir()) == ["a_example_1_20.png", "b_example_1_20.png"]
    assert [(f[0], f[2]) for f in exp.figures] == [("epoch_evol_per_param/a_example_1", 20), ("epoch_evol_per_param/b_example_1", 20)]
    assert exp.figures[0][1]._suptitle.get_text() == "a (K), t=4 (12 h) - epoch 20"
    assert not (tmp_path / "timestep_evol_per_param").exists()


def test_without_matplotlib_the_gif_is_still_written(tmp_path, monkeypatch):
    from PIL import Image

    from py4cast_amd import observers

    monkeypatch.setattr(observers, "_pyplot", lambda: None)
    monkeypatch.setattr(observers, "plasma_table", lambda: None)
    frames, vrange = _frames(3, 1, 6, 9)
    exp = Experiment()
    p = observers.PredictionTimestepPlot(1, save_path=tmp_path, lut=cf.synthetic_lut())
    assert p.table() is not None and observers.PredictionTimestepPlot(1).table() is None
    p.plotted_examples = 1
    p.plot_map(_obj(exp), frames, vrange, ["a"])
    assert exp.figures == [] and [f.name for f in (tmp_path / "timestep_evol_per_param").iterdir()] == ["a.gif"]
    with Image.open(tmp_path / "timestep_evol_per_param" / "a.gif") as gif:
        assert gif.n_frames == 3
    one = observers.PredictionTimestepPlot(1, save_path=tmp_path / "single", lut=cf.synthetic_lut())
    one.plot_map(_obj(exp), frames[:1], vrange, ["a"])        # one lead time: no GIF (plots.py:420)
    assert not (tmp_path / "single").exists()
    nowhere = observers.PredictionTimestepPlot(1, lut=cf.synthetic_lut())
    nowhere.plot_map(types.SimpleNamespace(), frames, vrange, ["a"])   # no save_path, no logger, no dataset_info: nothing raised


# ------------------------------------------------------------------------------------------------ Lightning
def test_lightning_builds_the_map_plotter_lists(tmp_path, monkeypatch):
    from helpers import make_dataset_info, register_test_models, synthetic_case
    from py4cast_amd import _lib
    from py4cast_amd.lightning import AutoRegressiveLightning
    from py4cast_amd.observers import PredictionEpochPlot, PredictionTimestepPlot, SpatialErrorPlot, StateErrorPlot

    def no_library():
        raise AssertionError("the library is not needed to build the plotters")

    register_test_models()
    case = synthetic_case(H=8, W=8, F=3)
    info = make_dataset_info(case, Ff=5)
    info.shortnames.setdefault("output", [])
    lm = AutoRegressiveLightning({}, info, None, model_name="TinyConvModel", num_pred_steps_val_test=3, num_samples_to_plot=3)
    lm.trainer = types.SimpleNamespace(logger=types.SimpleNamespace(log_dir=str(tmp_path)), precision="32-true")
    with pytest.warns(UserWarning):
        lm.setup("fit")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(AutoRegressiveLightning, "_reference_observers", staticmethod(lambda: (None, None)))
    lm.on_validation_start()
    lm.on_test_start()
    assert [type(p) for p in lm.valid_plotters] == [StateErrorPlot]                       # unchanged
    assert [type(p) for p in lm.test_plotters] == [StateErrorPlot, SpatialErrorPlot]
    assert [type(p) for p in lm.valid_map_plotters] == [PredictionTimestepPlot, PredictionEpochPlot]
    for p in lm.valid_map_plotters:                                                        # lightning.py:868-886
        assert (p.num_samples_to_plot, p.num_features_to_plot, p.prefix, p.save_path) == (1, 4, "Validation", tmp_path)
    (t,) = lm.test_map_plotters                                                            # lightning.py:1000-1015
    assert type(t) is PredictionTimestepPlot
    assert (t.num_samples_to_plot, t.num_features_to_plot, t.prefix, t.save_path) == (3, 4, "Test", tmp_path)
    # where the reference's plotters attach nothing changes: they sit in the old lists, the new ones stay empty
    ref = types.SimpleNamespace(PredictionTimestepPlot=lambda **kw: ("timestep", kw), PredictionEpochPlot=lambda **kw: ("epoch", kw))
    monkeypatch.setattr(AutoRegressiveLightning, "_reference_observers", staticmethod(lambda: (ref, None)))
    lm.on_validation_start()
    lm.on_test_start()
    assert [p[0] for p in lm.valid_plotters[1:]] == ["timestep", "epoch"] and [p[0] for p in lm.test_plotters[2:]] == ["timestep"]
    assert lm.valid_map_plotters == [] and lm.test_map_plotters == []
    # no logger: nothing is built
    monkeypatch.setattr(AutoRegressiveLightning, "_reference_observers", staticmethod(lambda: (None, None)))
    lm.trainer = None
    lm.on_validation_start()
    lm.on_test_start()
    assert lm.valid_plotters == [] and lm.test_plotters == [] and lm.valid_map_plotters == [] and lm.test_map_plotters == []
