"""GPU parity of the fused evaluation pass (p4c_eval_sums through ops.eval_sums) and of the native score-card / spatial-error
plotters: against the float64 closed form (tests/observers_closed_form.py) at rtol 1e-4 -- the project's fp32 parity bound
(README.md), every sum here being of non-negative terms -- with the masked count compared exactly; against the kernels the pass
replaces; against the reference's golden files through the plotter classes; and at the Lightning level."""

import json
import os
import types

import numpy as np
import pytest
import torch

import observers_closed_form as cf

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DIMS = ["batch", "timestep", "lat", "lon", "features"]
RTOL = 1e-4


def _have_matplotlib():
    try:
        import matplotlib  # noqa: F401

        return True
    except ImportError:
        return False


def _case(seed, shape, mask_kind="none", border=1):
    """prediction / target / mask on the CPU; NaN targets carry fully masked points inside and outside the interior"""
    g = torch.Generator().manual_seed(seed)
    S, F = shape[2:-1], shape[-1]
    p, t = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    interior = torch.ones(S)
    interior[:border], interior[-border:], interior[:, :border], interior[:, -border:] = 0, 0, 0, 0
    mask = None
    if mask_kind in ("f32", "u8"):
        mask = torch.rand(shape, generator=g) > 0.2
        mask[:, :, border, border + 1, :] = False       # masked for every (b,t,f): interior ...
        mask[:, :, 0, S[1] - 1, :] = False              # ... and border
        mask = mask.float() if mask_kind == "f32" else mask
    elif mask_kind == "nan":
        t[torch.rand(shape, generator=g) < 0.1] = float("nan")
        t[:, :, border, border + 1, :] = float("nan")
        t[:, :, S[0] - border - 1, border, :] = float("nan")
        t[:, :, 0, S[1] - 1, :] = float("nan")
        t[:, :, S[0] - 1, 0, :] = float("nan")
    return dict(p=p, t=t, mask=mask, kind=mask_kind, interior=interior, std=torch.rand(F, generator=g) + 0.5,
                w=torch.rand(F, generator=g) + 0.5)


def _spec(c, dev):
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    if c["kind"] == "nan":
        return ops.MaskSpec(L.MASK_FROM_NAN)
    return ops.MaskSpec.from_tensor(None if c["mask"] is None else c["mask"].to(dev))


def _run(c, dev, kind="MSELoss", pred=None, map_acc=None, accumulate=False, flatten=False):
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    p = c["p"].to(dev) if pred is None else pred
    t = c["t"].to(dev)
    if flatten:
        p, t = p.flatten(2, 3), t.flatten(2, 3)
    if map_acc is None:
        map_acc = torch.full((p.shape[1],) + tuple(p.shape[2:-1]), float("nan"), device=dev)   # overwritten, not added to
    interior = c["interior"].to(dev).reshape(-1)
    scores, count = ops.eval_sums(p, t, _spec(c, dev), c["std"].to(dev), interior, float(c["interior"].sum()), c["w"].to(dev),
                                  L.LOSS_MSE if kind == "MSELoss" else L.LOSS_L1, map_acc, accumulate)
    return scores, count, map_acc


def _closed(c, kind):
    mask = "nan" if c["kind"] == "nan" else c["mask"]
    return (cf.scores(c["p"], c["t"], mask, c["interior"], c["std"]), cf.masked_count(c["t"], mask),
            cf.loss_map(c["p"], c["t"], mask, c["w"], kind).sum(axis=0))


def _check(c, dev, kind, got=None):
    scores, count, amap = _run(c, dev, kind) if got is None else got
    want_scores, want_count, want_map = _closed(c, kind)
    assert scores.dtype == torch.float32 and scores.shape == want_scores.shape and count.dtype == torch.int32
    print("masked_count", int(count), want_count, "max rel score err",
          float(np.max(np.abs(scores.cpu().numpy() - want_scores) / want_scores)))
    assert int(count) == want_count
    np.testing.assert_allclose(scores.cpu().numpy(), want_scores, rtol=RTOL, atol=0)
    np.testing.assert_allclose(amap.cpu().numpy().reshape(want_map.shape), want_map, rtol=RTOL, atol=0)


# where the kernel can go wrong: several workgroups + tails + the 16-byte path; lanes straddling points; N*F % 4 != 0 (scalar path);
# F = 3; F = 68 (two feature iterations); B = T = 1; two tiles per workgroup (N > 64 * 1024)
SHAPES = {
    "big_16B": ((3, 4, 96, 130, 60), "none", "MSELoss"),
    "straddle_F21": ((2, 2, 8, 12, 21), "f32", "L1Loss"),
    "scalar_F21": ((2, 2, 7, 9, 21), "nan", "MSELoss"),
    "F3": ((2, 3, 10, 12, 3), "u8", "MSELoss"),
    "F68": ((2, 2, 6, 10, 68), "f32", "L1Loss"),
    "B1_T1": ((1, 1, 16, 24, 8), "none", "L1Loss"),
    "two_tiles": ((1, 2, 300, 512, 4), "nan", "MSELoss"),
    "two_tiles_scalar": ((1, 1, 257, 511, 3), "u8", "L1Loss"),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_eval_sums_matches_closed_form(name, gpu_device):
    shape, mask_kind, kind = SHAPES[name]
    _check(_case(11, shape, mask_kind), gpu_device, kind)


@pytest.mark.parametrize("shape", [(2, 2, 12, 20, 12), (2, 2, 7, 9, 5)], ids=["flat", "scalar"])
@pytest.mark.parametrize("mask_kind", ["none", "nan", "f32", "u8"])
def test_eval_sums_four_mask_modes(mask_kind, shape, gpu_device):
    c = _case(12, shape, mask_kind, border=2)
    _check(c, gpu_device, "MSELoss")
    if mask_kind != "none":   # fully masked points inside and outside the interior are counted alike
        assert cf.masked_count(c["t"], "nan" if mask_kind == "nan" else c["mask"]) >= 2


def test_eval_sums_strided_and_misaligned_views(gpu_device):
    c = _case(13, (2, 2, 8, 12, 20), "nan")
    big = torch.zeros(3, 5, 8, 12, 20, device=gpu_device)
    big[1:3, 2:4] = c["p"].to(gpu_device)
    view = big[1:3, 2:4]
    assert not view.is_contiguous()
    _check(c, gpu_device, "MSELoss", got=_run(c, gpu_device, "MSELoss", pred=view))
    # a base 4 bytes off the 16-byte grid: the scalar path on a shape the flat path would take
    flat = torch.zeros(c["p"].numel() + 1, device=gpu_device)
    flat[1:] = c["p"].to(gpu_device).reshape(-1)
    off = flat[1:].view(c["p"].shape)
    assert off.data_ptr() % 16 == 4
    got = _run(c, gpu_device, "MSELoss", pred=off)
    _check(c, gpu_device, "MSELoss", got=got)
    # a time stride off the 16-byte grid (F = 3, odd row count): the scalar path again
    c3 = _case(14, (2, 2, 5, 8, 3), "f32")
    big3 = torch.zeros(2, 2, 5 * 8 * 3 + 1, device=gpu_device)
    big3[:, :, :120] = c3["p"].to(gpu_device).reshape(2, 2, 120)
    _check(c3, gpu_device, "L1Loss", got=_run(c3, gpu_device, "L1Loss", pred=big3[:, :, :120].view(2, 2, 5, 8, 3)))


def test_flattened_call_equals_grid_call(gpu_device):
    c = _case(15, (2, 3, 12, 20, 12), "nan")
    a, b = _run(c, gpu_device, "MSELoss"), _run(c, gpu_device, "MSELoss", flatten=True)
    assert b[2].shape == (3, 240)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].flatten(1), b[2])


@pytest.mark.parametrize("name", ["big_16B", "scalar_F21", "straddle_F21"])
def test_eval_sums_matches_the_kernels_it_replaces(name, gpu_device):
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    shape, mask_kind, kind = SHAPES[name]
    c = _case(16, shape, mask_kind)
    scores, count, amap = _run(c, gpu_device, kind)
    p, t, spec = c["p"].to(gpu_device), c["t"].to(gpu_device), _spec(c, gpu_device)
    interior, num_interior = c["interior"].to(gpu_device).reshape(-1), float(c["interior"].sum())
    old_count = ops.masked_count(spec, t)
    assert int(count) == (0 if old_count is None else int(old_count))
    for i, code in enumerate((L.LOSS_L1, L.LOSS_MSE)):
        old = ops.scaled_loss(p, t, spec, c["std"].to(gpu_device), interior, num_interior, code, count=old_count)
        np.testing.assert_allclose(scores[i].cpu().numpy(), old.cpu().numpy(), rtol=RTOL, atol=0)
    old_map = ops.weighted_loss_map(p, t, spec, c["w"].to(gpu_device), L.LOSS_MSE if kind == "MSELoss" else L.LOSS_L1).sum(0)
    np.testing.assert_allclose(amap.cpu().numpy(), old_map.cpu().numpy(), rtol=RTOL, atol=0)


@pytest.mark.parametrize("shape", [(2, 2, 12, 20, 12), (2, 2, 7, 9, 5)], ids=["flat", "scalar"])
def test_accumulate_and_equal_bits(shape, gpu_device):
    from py4cast_amd import ops

    c = _case(17, shape, "nan")
    s1, n1, m1 = _run(c, gpu_device, "L1Loss")
    s2, n2, m2 = _run(c, gpu_device, "L1Loss")
    assert torch.equal(s1, s2) and torch.equal(n1, n2) and torch.equal(m1, m2)          # two calls: equal bits
    acc = torch.zeros_like(m1)
    _run(c, gpu_device, "L1Loss", map_acc=acc, accumulate=True)
    assert torch.equal(acc, m1)                                                         # 0 + map
    _run(c, gpu_device, "L1Loss", map_acc=acc, accumulate=True)
    np.testing.assert_allclose(acc.cpu().numpy(), 2 * m1.cpu().numpy(), rtol=RTOL, atol=0)
    # no map asked: the scores and the count are the same bits, nothing else is written
    s3, n3 = ops.eval_sums(c["p"].to(gpu_device), c["t"].to(gpu_device), _spec(c, gpu_device), c["std"].to(gpu_device),
                           c["interior"].to(gpu_device).reshape(-1), float(c["interior"].sum()), None, None)
    assert torch.equal(s3, s1) and torch.equal(n3, n1)


# ------------------------------------------------------------------------------------------------ the plotter classes
class Experiment:
    def __init__(self):
        self.scalars, self.figures = [], []

    def add_scalar(self, name, value, step):
        self.scalars.append((name, float(value), int(step)))

    def add_figure(self, name, fig, step):
        self.figures.append((name, fig, int(step)))


def _golden_obj(z, dev, exp):
    from py4cast_amd.base import Stats
    from py4cast_amd.losses import ScaledLoss, WeightedLoss

    names = [str(n) for n in z["names"]]
    info = types.SimpleNamespace(
        state_weights={n: float(z["state_weight"][i]) for i, n in enumerate(names)},
        stats=Stats({n: {"std": torch.tensor(z["std"][i]), "mean": torch.tensor(0.0)} for i, n in enumerate(names)}),
        diff_stats=Stats({n: {"std": torch.tensor(z["diff_std"][i]), "mean": torch.tensor(0.0)} for i, n in enumerate(names)}),
        units={n: str(u) for n, u in zip(names, z["units"])}, pred_step=1)
    lm = torch.nn.Module()
    interior = torch.from_numpy(z["interior"]).to(dev)
    metrics = {}
    for torch_loss, alias in ("L1Loss", "mae"), ("MSELoss", "rmse"):
        metrics[alias] = ScaledLoss(torch_loss, reduction="none")
        metrics[alias].prepare(lm, interior, info)
    loss = WeightedLoss(str(z["map_loss"]), reduction="none")
    loss.prepare(lm, interior, info)
    trainer = types.SimpleNamespace(is_global_zero=True, sanity_checking=False, logger=types.SimpleNamespace(experiment=exp))
    obj = types.SimpleNamespace(loss=loss, dataset_info=info, trainer=trainer, interior_2d=interior, current_epoch=0, grid_shape=interior.shape[:2])
    return obj, metrics, names


@pytest.mark.parametrize("name,lazy,linked", [("case0", False, True), ("case1", False, True), ("case2", False, True), ("case2", True, False)])
def test_golden_cases_through_the_native_plotters(name, lazy, linked, gpu_device, tmp_path, monkeypatch):
    """per-update scores and maps, final means, mean map, scalar names and JSON of the reference's run; ``lazy``: the NaN case as
    the Lightning module hands it over (raw target + NanMask marker); ``linked``: one pass for both plotters"""
    from py4cast_amd import observers, ops
    from py4cast_amd.losses import NanMask
    from py4cast_amd.namedtensor import NamedTensor

    z = np.load(os.path.join(GOLD, f"observers_{name}.npz"))
    exp = Experiment()
    obj, metrics, names = _golden_obj(z, gpu_device, exp)
    state, spatial = observers.StateErrorPlot(metrics, prefix="Test", save_path=tmp_path), observers.SpatialErrorPlot(prefix="Test")
    if linked:
        state.map_consumer = spatial
    calls, eval_sums = [], ops.eval_sums
    monkeypatch.setattr(observers.ops, "eval_sums", lambda *a, **k: (calls.append(1), eval_sums(*a, **k))[1])
    map_sum = 0.0
    for u in range(2):
        p = NamedTensor(torch.from_numpy(z[f"pred{u}"]).to(gpu_device), DIMS, names)
        raw = torch.from_numpy(z[f"target{u}"]).to(gpu_device)
        if lazy:
            t, mask = NamedTensor(raw, DIMS, names), NanMask(raw)
        else:
            t, mask = NamedTensor(torch.nan_to_num(raw, nan=0), DIMS, names), torch.from_numpy(z[f"mask{u}"]).to(gpu_device)
        state.update(obj, None, p, t, mask)
        scores = observers._LAST_STEP[0]["scores"].cpu().numpy()
        spatial.update(obj, None, p, t, mask)
        np.testing.assert_allclose(scores[0], z[f"mae{u}"], rtol=RTOL, atol=0)
        np.testing.assert_allclose(scores[1], z[f"rmse{u}"], rtol=RTOL, atol=0)
        map_sum = map_sum + z[f"map{u}"].astype(np.float64).sum(axis=0)
        np.testing.assert_allclose(spatial.map_acc.cpu().numpy(), map_sum, rtol=RTOL, atol=0)
        assert state.sums["mae"].is_cuda and state.sums["mae"].dtype == torch.float64 and spatial.map_acc.is_cuda
    assert len(calls) == (2 if linked else 4) and state.count == spatial.count == 2 * z["pred0"].shape[0]
    state.on_step_end(obj, label="Test")
    spatial.on_step_end(obj, label="Test")
    np.testing.assert_allclose(state.last_means["mae"].numpy(), z["mean_mae"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(state.last_means["rmse"].numpy(), z["mean_rmse"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(spatial.last_mean_map.numpy(), z["mean_map"], rtol=RTOL, atol=0)
    assert [s[0] for s in exp.scalars] == [str(s) for s in z["scalar_names"]]
    assert [s[2] for s in exp.scalars] == [int(s) for s in z["scalar_steps"]]
    np.testing.assert_allclose([s[1] for s in exp.scalars], z["scalar_values"], rtol=RTOL, atol=0)
    for alias in ("mae", "rmse"):
        got, want = json.loads((tmp_path / f"Test_{alias}_scores.json").read_text()), json.loads(str(z[f"json_{alias}"]))
        assert list(got) == list(want) == names
        np.testing.assert_allclose([got[n] for n in names], [want[n] for n in names], rtol=RTOL, atol=0)
    if _have_matplotlib():   # the reference's figure names and steps
        assert [f[0] for f in exp.figures] == [str(n) for n in z["figure_names"]]
        assert [f[2] for f in exp.figures] == [int(s) for s in z["figure_steps"]]
        assert [f[1]._suptitle.get_text() for f in exp.figures[2:]] == [str(s) for s in z["spatial_titles"]]
    else:
        assert exp.figures == []


# ------------------------------------------------------------------------------------------------ the Lightning level
def _module(gpu_device, tmp_path, exp, case):
    from helpers import make_dataset_info, register_test_models
    from py4cast_amd.lightning import AutoRegressiveLightning

    register_test_models()
    info = make_dataset_info(case, Ff=5)
    info.shortnames.setdefault("output", [])
    lm = AutoRegressiveLightning({}, info, None, num_input_steps=1, num_pred_steps_train=3, num_pred_steps_val_test=3, batch_size=2,
                                 model_name="TinyConvModel")
    with torch.no_grad():
        g = torch.Generator().manual_seed(9)
        lm.model.w.copy_(torch.randn(lm.model.w.shape, generator=g) * 0.1)
        lm.model.b.copy_(torch.randn(lm.model.b.shape, generator=g) * 0.1)
    lm = lm.to(gpu_device)
    lm.trainer = types.SimpleNamespace(logger=types.SimpleNamespace(log_dir=str(tmp_path), experiment=exp), precision="32-true")
    lm.log_dict = lambda d, **kw: None
    with pytest.warns(UserWarning):
        lm.setup("test")
    return lm, info


def _closed_epoch(lm, cases, dev):
    from helpers import make_batch

    preds, targets = [], []
    for case in cases:
        with torch.no_grad():
            pred, target = lm.common_step(make_batch(case, dev), 0, phase="val_test")
        preds.append(pred.tensor.cpu()), targets.append(target.tensor.cpu())
    return torch.cat(preds), torch.cat(targets)


def test_test_epoch_yields_scalars_json_and_spatial_figures(gpu_device, tmp_path):
    """setup -> on_test_start -> two test_step calls -> on_test_epoch_end, no py4cast package involved: fails on a tree where no
    plotter attaches"""
    from helpers import make_batch, synthetic_case

    cases = [synthetic_case(seed=s, B=2, T=3, H=16, W=24, F=3, border=2) for s in (3, 4)]
    exp = Experiment()
    lm, info = _module(gpu_device, tmp_path, exp, cases[0])
    calls = []
    from py4cast_amd import observers, ops

    eval_sums = ops.eval_sums
    observers.ops.eval_sums = lambda *a, **k: (calls.append(1), eval_sums(*a, **k))[1]
    try:
        lm.on_test_start()
        for i, case in enumerate(cases):
            lm.test_step(make_batch(case, gpu_device), i)
        lm.on_test_epoch_end()
    finally:
        observers.ops.eval_sums = eval_sums
    assert len(calls) == 2                                        # one pass per step for both plotters
    names, T = info.shortnames["input_output"], 3
    pred, target = _closed_epoch(lm, cases, gpu_device)
    interior = 1.0 - cases[0]["border_mask"][..., 0]
    want = cf.scores(pred, target, None, interior, cases[0]["std"]).mean(axis=1)      # (2,T,F): mean over the 4 samples
    assert [(s[0], s[2]) for s in exp.scalars] == [(f"Test_{a}/timestep_{n}", t + 1) for a in ("mae", "rmse") for t in range(T) for n in names]
    np.testing.assert_allclose(np.array([s[1] for s in exp.scalars]).reshape(2, T, len(names)), want, rtol=RTOL, atol=0)
    for i, alias in enumerate(("mae", "rmse")):
        d = json.loads((tmp_path / f"Test_{alias}_scores.json").read_text())
        assert list(d) == names
        np.testing.assert_allclose(np.array([d[n] for n in names]).T, want[i], rtol=RTOL, atol=0)
    w = cf.weights(cases[0]["state_weight"], cases[0]["diff_std"], "MSELoss")
    want_map = cf.loss_map(pred, target, None, w, "MSELoss").mean(axis=0)
    np.testing.assert_allclose(lm.test_plotters[1].last_mean_map.numpy(), want_map, rtol=RTOL, atol=0)
    spatial = [f for f in exp.figures if f[0] == "spatial_error_Test/Test_loss"]
    if _have_matplotlib():
        assert [f[2] for f in spatial] == list(range(T))
        assert {f[0] for f in exp.figures} >= {"score_cards/Test_mae", "score_cards/Test_rmse"}
        assert (tmp_path / "score_cards" / "Test_rmse.png").stat().st_size > 0
    else:
        assert spatial == []


def test_validation_epoch_yields_mae_scalars(gpu_device, tmp_path):
    from helpers import make_batch, synthetic_case

    case = synthetic_case(seed=5, B=2, T=3, H=16, W=24, F=3, border=1)
    exp = Experiment()
    lm, info = _module(gpu_device, tmp_path, exp, case)
    lm.on_validation_start()
    lm.validation_step(make_batch(case, gpu_device), 0)
    lm.on_validation_epoch_end()
    names, T = info.shortnames["input_output"], 3
    assert [(s[0], s[2]) for s in exp.scalars] == [(f"Valid_mae/timestep_{n}", t + 1) for t in range(T) for n in names]
    pred, target = _closed_epoch(lm, [case], gpu_device)
    want = cf.scores(pred, target, None, 1.0 - case["border_mask"][..., 0], case["std"])[0].mean(axis=0)
    np.testing.assert_allclose(np.array([s[1] for s in exp.scalars]).reshape(T, len(names)), want, rtol=RTOL, atol=0)
    assert not any(f[0].startswith("spatial_error") for f in exp.figures)
    assert lm.valid_plotters[0].count == 0
