"""Score-card and spatial-error observers, the parts that need no GPU: the float64 closed form against the reference's golden files,
the two new ABI symbols, the merge of the ranks' states, and the host logic of ``on_step_end`` (scalars, JSON, figures, sanity
checking, missing attributes) on hand-made CPU state with a recording fake ``experiment``."""

import json
import os
import types

import numpy as np
import pytest
import torch

import observers_closed_form as cf

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = ["case0", "case1", "case2"]


def _load(name):
    return np.load(os.path.join(GOLD, f"observers_{name}.npz"))


def _mask(z, u):
    """the closed form's mask argument: the NaN case is told by the raw target itself"""
    return "nan" if np.isnan(z[f"target{u}"]).any() else z[f"mask{u}"]


def _have_matplotlib():
    try:
        import matplotlib  # noqa: F401

        return True
    except ImportError:
        return False


class Experiment:
    def __init__(self):
        self.scalars, self.figures = [], []

    def add_scalar(self, name, value, step):
        self.scalars.append((name, float(value), int(step)))

    def add_figure(self, name, fig, step):
        self.figures.append((name, fig, int(step)))


def test_golden_cases_cover_what_they_should():
    z0, z1, z2 = (_load(c) for c in CASES)
    assert (z0["mask0"] == 1).all() and not np.isnan(z0["target0"]).any()
    assert z1["mask0"].dtype == np.float32 and 0 < (z1["mask0"] == 0).mean() < 0.5
    interior = z2["interior"][..., 0]
    for u in range(2):
        gone = np.isnan(z2[f"target{u}"]).all(axis=(0, 1, 4))
        assert (gone & (interior == 1)).any() and (gone & (interior == 0)).any()     # fully masked points inside and outside
        assert cf.masked_count(z2[f"target{u}"], "nan") == gone.sum() == 2 + u
    assert {str(z["map_loss"]) for z in (z0, z1, z2)} == {"MSELoss", "L1Loss"}


@pytest.mark.parametrize("name", CASES)
def test_closed_form_reproduces_reference(name):
    """the goldens are the reference's float32 results: fp32 sums of at most 240 non-negative terms, <= 1e-5 from float64"""
    z = _load(name)
    kind = str(z["map_loss"])
    w = cf.weights(z["state_weight"], z["diff_std"], kind)
    per = {"mae": [], "rmse": [], "map": []}
    for u in range(2):
        s = cf.scores(z[f"pred{u}"], z[f"target{u}"], _mask(z, u), z["interior"], z["std"])
        m = cf.loss_map(z[f"pred{u}"], z[f"target{u}"], _mask(z, u), w, kind)
        np.testing.assert_allclose(s[0], z[f"mae{u}"], rtol=1e-5)
        np.testing.assert_allclose(s[1], z[f"rmse{u}"], rtol=1e-5)
        np.testing.assert_allclose(m, z[f"map{u}"], rtol=1e-5, atol=1e-7)
        per["mae"].append(s[0]), per["rmse"].append(s[1]), per["map"].append(m)
    np.testing.assert_allclose(cf.epoch_means(per["mae"]), z["mean_mae"], rtol=1e-5)
    np.testing.assert_allclose(cf.epoch_means(per["rmse"]), z["mean_rmse"], rtol=1e-5)
    np.testing.assert_allclose(cf.epoch_means(per["map"]), z["mean_map"], rtol=1e-5, atol=1e-7)
    # the scalars and the JSON files are these means, feature by feature and lead time by lead time
    names, T = [str(n) for n in z["names"]], z["mean_mae"].shape[0]
    want = [(f"Test_{a}/timestep_{n}", t + 1) for a in ("mae", "rmse") for t in range(T) for n in names]
    assert list(zip((str(s) for s in z["scalar_names"]), (int(s) for s in z["scalar_steps"]))) == want
    np.testing.assert_allclose(z["scalar_values"], np.concatenate([z["mean_mae"].ravel(), z["mean_rmse"].ravel()]), rtol=1e-6)
    for alias in ("mae", "rmse"):
        d = json.loads(str(z[f"json_{alias}"]))
        assert list(d) == names
        np.testing.assert_allclose(np.array([d[n] for n in names]).T, z[f"mean_{alias}"], rtol=1e-6)


def test_abi_gains_the_two_functions():
    from py4cast_amd import _lib

    handle = _lib.lib()
    for name in ("p4c_eval_sums", "p4c_eval_sums_workspace_bytes"):
        assert name in _lib.all_symbols() and hasattr(handle, name)
    assert len(_lib.SIGNATURES["p4c_eval_sums"]) == 23
    ws = handle.p4c_eval_sums_workspace_bytes
    assert ws(2, 3, 64, 5) == (2 * 2 * 3 * 5 + 1) * 4                     # one workgroup of 64 grid points
    assert ws(2, 3, 65, 5) == (2 * 2 * 3 * 5 + 1) * 2 * 4
    assert ws(1, 1, 512 * 512, 60) == (2 * 60 + 1) * 1024 * 4             # 256 grid points per workgroup
    assert ws(1, 1, 1 << 22, 1) == 3 * ((1 << 22) // 512) * 4             # at most 512 grid points per workgroup
    assert ws(0, 1, 64, 5) == 0


def test_eval_sums_has_no_cpu_path():
    from py4cast_amd import _lib, ops

    x = torch.zeros(1, 1, 4, 4, 2)
    with pytest.raises(_lib.P4CError):
        ops.eval_sums(x, x, ops.MaskSpec(0), torch.ones(2), torch.ones(16), 16.0, None, None)


def test_two_ranks_states_give_the_global_mean():
    from py4cast_amd.observers import merge_mean, pack_state

    g = torch.Generator().manual_seed(5)
    T, F, S = 3, 4, (5, 6)
    # per rank: two steps of B = 2 samples -> per-sample scores (B,T,F) and maps (B,T,*S)
    ranks = [[(torch.rand(2, T, F, generator=g, dtype=torch.float64), torch.rand(2, T, *S, generator=g)) for _ in range(2)] for _ in range(2)]
    flats = []
    for steps in ranks:
        sums = sum(s.sum(0) for s, _ in steps)
        maps = sum(m.sum(0) for _, m in steps)
        flats.append(pack_state([sums, maps], sum(s.shape[0] for s, _ in steps)))
    assert flats[0].dtype == torch.float64 and flats[0].shape == (T * F + T * 30 + 1,)
    mean_s, mean_m = merge_mean(flats[0] + flats[1], [(T, F), (T,) + S])
    # the reference: mean over ranks of each step's tensor, then the mean over the concatenated batches
    ref_s = torch.cat([(ranks[0][i][0] + ranks[1][i][0]) / 2 for i in range(2)]).mean(0)
    ref_m = torch.cat([(ranks[0][i][1] + ranks[1][i][1]) / 2 for i in range(2)]).mean(0)
    assert mean_s.shape == (T, F) and mean_m.shape == (T,) + S
    np.testing.assert_allclose(mean_s.numpy(), ref_s.numpy(), rtol=1e-12)
    np.testing.assert_allclose(mean_m.numpy(), ref_m.double().numpy(), rtol=1e-6)
    # one rank alone: its own mean
    (alone,) = merge_mean(pack_state([torch.full((2, 2), 6.0)], 3), [(2, 2)])
    assert torch.equal(alone, torch.full((2, 2), 2.0, dtype=torch.float64))


def _hand_made(tmp_path, T=3, names=("a", "b")):
    from py4cast_amd.observers import SpatialErrorPlot, StateErrorPlot

    state = StateErrorPlot({"mae": None, "rmse": None}, prefix="Test", save_path=tmp_path)
    state.shortnames, state.units, state.initialized = list(names), ["K", ""], True
    mae = torch.arange(T * len(names), dtype=torch.float64).reshape(T, len(names)) + 1.0
    state.sums, state.count = {"mae": mae * 4, "rmse": mae * 8}, 4
    spatial = SpatialErrorPlot(prefix="Test")
    spatial.map_acc, spatial.count = torch.arange(T * 6 * 8, dtype=torch.float32).reshape(T, 6, 8) * 4, 4
    return state, spatial, mae


def _obj(experiment=None, sanity=False, **extra):
    interior = torch.ones(6, 8, 1)
    interior[0] = 0
    trainer = types.SimpleNamespace(is_global_zero=True, sanity_checking=sanity)
    logger = None if experiment is None else types.SimpleNamespace(experiment=experiment)
    return types.SimpleNamespace(trainer=trainer, logger=logger, interior_2d=interior, current_epoch=7,
                                 dataset_info=types.SimpleNamespace(units=None, pred_step=3.0), **extra)


def test_on_step_end_scalars_json_and_figures(tmp_path):
    exp = Experiment()
    state, spatial, mae = _hand_made(tmp_path)
    obj = _obj(exp)
    state.on_step_end(obj, label="Test")
    spatial.on_step_end(obj, label="Test")
    want = [(f"Test_{a}/timestep_{n}", float(k * mae[t, i]), t + 1)
            for a, k in (("mae", 1), ("rmse", 2)) for t in range(3) for i, n in enumerate(("a", "b"))]
    assert exp.scalars == want
    for alias, k in ("mae", 1), ("rmse", 2):
        d = json.loads((tmp_path / f"Test_{alias}_scores.json").read_text())
        assert d == {"a": [float(k * mae[t, 0]) for t in range(3)], "b": [float(k * mae[t, 1]) for t in range(3)]}
    np.testing.assert_array_equal(spatial.last_mean_map.numpy(), np.arange(3 * 6 * 8, dtype=np.float64).reshape(3, 6, 8))
    # the state is cleared: a second end of epoch has nothing to say
    assert state.count == 0 and state.sums == {} and spatial.count == 0 and spatial.map_acc is None
    state.on_step_end(obj, label="Test")
    spatial.on_step_end(obj, label="Test")
    assert len(exp.scalars) == len(want)
    names = [f[0] for f in exp.figures]
    if _have_matplotlib():
        assert names == ["score_cards/Test_mae", "score_cards/Test_rmse"] + ["spatial_error_Test/Test_loss"] * 3
        assert [f[2] for f in exp.figures] == [7, 7, 0, 1, 2]
        for alias in ("mae", "rmse"):
            assert (tmp_path / "score_cards" / f"Test_{alias}.png").stat().st_size > 0
        card = exp.figures[0][1].axes[0]
        assert [t.get_text() for t in card.get_yticklabels()] == ["a (K)", "b"]
        assert [t.get_text() for t in card.get_xticklabels()] == ["3.0", "6.0", "9.0"]
        assert sorted(t.get_text() for t in card.texts) == sorted(f"{v:.3f}" for v in mae.numpy().ravel())
        assert exp.figures[3][1]._suptitle.get_text() == "Test loss, t=1 (3.0 h)"
        shown = exp.figures[2][1].axes[0].images[0]
        np.testing.assert_array_equal(np.asarray(shown.get_array()), np.arange(48.0).reshape(6, 8))
        assert np.asarray(shown.get_alpha())[0, 0] == 0.7 and np.asarray(shown.get_alpha())[1, 0] == 1.0   # the border shows through
    else:
        assert names == [] and not (tmp_path / "score_cards").exists()


def test_figures_are_skipped_without_matplotlib(tmp_path, monkeypatch):
    from py4cast_amd import observers

    monkeypatch.setattr(observers, "_pyplot", lambda: None)
    exp = Experiment()
    state, spatial, _ = _hand_made(tmp_path)
    state.on_step_end(_obj(exp), label="Test")
    spatial.on_step_end(_obj(exp), label="Test")
    assert len(exp.scalars) == 12 and exp.figures == [] and not (tmp_path / "score_cards").exists()
    assert (tmp_path / "Test_mae_scores.json").exists() and (tmp_path / "Test_rmse_scores.json").exists()
    assert spatial.last_mean_map.shape == (3, 6, 8)


def test_nothing_written_while_sanity_checking(tmp_path):
    exp = Experiment()
    state, spatial, _ = _hand_made(tmp_path)
    obj = _obj(exp, sanity=True)
    state.on_step_end(obj, label="Valid")
    spatial.on_step_end(obj, label="Valid")
    assert len(exp.scalars) == 12 and all(s[0].startswith("Valid_") for s in exp.scalars)   # the reference logs the scalars there too
    assert exp.figures == [] and list(tmp_path.iterdir()) == []
    assert state.count == 0 and spatial.count == 0


def test_missing_attributes_do_not_raise(tmp_path):
    """no logger, no trainer flags, no units, no mlflow_logger, no save_path: what the existing tests' SimpleNamespace trainer has"""
    from py4cast_amd.observers import StateErrorPlot

    state, spatial, mae = _hand_made(tmp_path)
    bare = types.SimpleNamespace(trainer=types.SimpleNamespace(logger=types.SimpleNamespace(log_dir=str(tmp_path))))
    state.on_step_end(bare, label="Test")
    spatial.on_step_end(bare, label="Test")
    assert json.loads((tmp_path / "Test_mae_scores.json").read_text())["a"] == [float(mae[t, 0]) for t in range(3)]
    np.testing.assert_array_equal(state.last_means["rmse"].numpy(), 2 * mae.numpy())
    nowhere = StateErrorPlot({"mae": None})
    nowhere.shortnames, nowhere.units, nowhere.sums, nowhere.count = ["a", "b"], ["", ""], {"mae": mae.clone()}, 1
    nowhere.on_step_end(types.SimpleNamespace(), label="Test")
    assert nowhere.count == 0
    # a rank other than zero reduces and clears, and writes nothing
    state, spatial, _ = _hand_made(tmp_path / "other")
    exp = Experiment()
    obj = _obj(exp)
    obj.trainer.is_global_zero = False
    state.on_step_end(obj, label="Test")
    spatial.on_step_end(obj, label="Test")
    assert exp.scalars == [] and exp.figures == [] and not (tmp_path / "other").exists() and state.count == 0


def test_mlflow_logger_receives_the_figures(tmp_path):
    logged = []
    mlflow = types.SimpleNamespace(version="run7", experiment=types.SimpleNamespace(
        log_figure=lambda run_id, figure, artifact_file: logged.append((run_id, artifact_file))))
    state, spatial, _ = _hand_made(tmp_path)
    obj = _obj(None, mlflow_logger=mlflow)
    state.on_step_end(obj, label="Test")
    spatial.on_step_end(obj, label="Test")
    want = [("run7", "figures/score_cards/Test_mae.png"), ("run7", "figures/score_cards/Test_rmse.png")] + \
        [("run7", "figures/spatial_error_Test/Test_loss.png")] * 3
    assert logged == (want if _have_matplotlib() else [])


def test_unfused_combinations_call_the_objects_as_the_reference_does():
    """a metric that is no ScaledLoss, a loss that is no single WeightedLoss: the plotters call them and keep the same state"""
    from py4cast_amd.namedtensor import NamedTensor
    from py4cast_amd.observers import SpatialErrorPlot, StateErrorPlot

    dims, names = ["batch", "timestep", "lat", "lon", "features"], ["a", "b"]
    calls = []

    def metric(prediction, target, mask):
        calls.append("metric")
        return (prediction.tensor - target.tensor).abs().mean(dim=(2, 3))

    def loss(prediction, target, mask, reduce_spatial_dim=True):
        calls.append(("loss", reduce_spatial_dim))
        return (prediction.tensor - target.tensor).abs().sum(-1)

    obj = types.SimpleNamespace(loss=loss, dataset_info=types.SimpleNamespace(units={"a": "K"}))
    state, spatial = StateErrorPlot({"custom": metric}), SpatialErrorPlot()
    g = torch.Generator().manual_seed(1)
    batches = [(torch.randn(2, 3, 4, 5, 2, generator=g), torch.randn(2, 3, 4, 5, 2, generator=g)) for _ in range(2)]
    for p, t in batches:
        pn, tn = NamedTensor(p, dims, names), NamedTensor(t, dims, names)
        state.update(obj, None, pn, tn, None)
        spatial.update(obj, None, pn, tn, None)
    assert calls == ["metric", ("loss", False)] * 2 and state.count == 4 and spatial.count == 4
    assert state.units == ["K", ""] and state.sums["custom"].dtype == torch.float64 and spatial.map_acc.shape == (3, 4, 5)
    state.on_step_end(obj, label="Test")
    spatial.on_step_end(obj, label="Test")
    allp, allt = torch.cat([b[0] for b in batches]), torch.cat([b[1] for b in batches])
    np.testing.assert_allclose(state.last_means["custom"].numpy(), (allp - allt).abs().mean(dim=(2, 3)).mean(0).numpy(), rtol=1e-6)
    np.testing.assert_allclose(spatial.last_mean_map.numpy(), (allp - allt).abs().sum(-1).mean(0).numpy(), rtol=1e-6)


def test_lightning_attaches_the_native_plotters(tmp_path):
    from helpers import make_dataset_info, register_test_models, synthetic_case
    from py4cast_amd.lightning import AutoRegressiveLightning
    from py4cast_amd.observers import SpatialErrorPlot, StateErrorPlot

    register_test_models()
    case = synthetic_case(H=8, W=8, F=3)
    info = make_dataset_info(case, Ff=5)
    info.shortnames.setdefault("output", [])
    lm = AutoRegressiveLightning({}, info, None, model_name="TinyConvModel", num_pred_steps_val_test=3)
    lm.trainer = types.SimpleNamespace(logger=types.SimpleNamespace(log_dir=str(tmp_path)), precision="32-true")
    with pytest.warns(UserWarning):
        lm.setup("fit")
    lm.on_validation_start()
    lm.on_test_start()
    assert [type(p) for p in lm.valid_plotters] == [StateErrorPlot]
    assert list(lm.valid_plotters[0].metrics) == ["mae"] and lm.valid_plotters[0].prefix == "Validation"
    assert [type(p) for p in lm.test_plotters] == [StateErrorPlot, SpatialErrorPlot]
    state, spatial = lm.test_plotters
    assert list(state.metrics) == ["mae", "rmse"] and state.save_path == tmp_path and state.map_consumer is spatial
    assert [m.loss_name for m in state.metrics.values()] == ["L1Loss", "MSELoss"] and spatial.prefix == "Test"
    lm.trainer = None
    lm.on_validation_start()
    lm.on_test_start()
    assert lm.valid_plotters == [] and lm.test_plotters == []
