"""
The native rollout beyond one model call per target step and beyond training (HalfUNetMI355X.native_rollout):
  * num_inter_steps = K >= 2 (scaled_ar): a schedule of T * K model calls, the first K - 1 of every target step FREE steps
    (p4c_ar_update_next / p4c_out_conv_update_fwd: border forced to the target, no loss, state in scratch), the K-th the loss step;
  * phase "inference": a forward-only forecast of free steps without border forcing.
Checked against the generic per-op path on the same kernels (``lm.use_native_rollout = False``), with the bars of
tests/test_wide_rollout_gpu.py; the launches of each route are counted by wrapping ``_lib.call``.
The float64 check of these schedules, call by call, is tests/test_rollout_nodes_gpu.py.
"""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = {"compute_dtype": "bf16", "activation_dtype": "bf16"}
FREE = ("p4c_out_conv_update_fwd", "p4c_ar_update_next")


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _case(nan=False, **kw):
    """helpers.synthetic_case; its NaN pattern needs T >= 2, so the same NaNs are planted here for any T: one in the input state,
    one in the forcing, a grid point whose target is NaN in every feature, and a single NaN target element."""
    from helpers import synthetic_case

    case = synthetic_case(nan=False, **kw)
    if nan:
        case["inputs"][0, 0, 3, 4, 1] = float("nan")
        case["forcing"][-1, -1, 5, 6, 2] = float("nan")
        case["outputs"][:, :, 7, 8, :] = float("nan")
        case["outputs"][0, -1, 2, 2, 0] = float("nan")
    return case


def _lm(case, T_in, T, K, strategy, nan, device, settings=None, weight=0.7):
    from helpers import make_dataset_info
    from py4cast_amd.lightning import AutoRegressiveLightning

    info = make_dataset_info(case, case["forcing"].shape[-1])
    torch.manual_seed(0)
    return AutoRegressiveLightning(
        settings or {}, info, None, num_input_steps=T_in, num_pred_steps_train=T, batch_size=2, model_name="HalfUNet",
        losses=[{"class": "WeightedLoss", "weight": weight, "params": {"loss": "MSELoss", "reduction": "none"}}],
        training_strategy=strategy, mask_on_nan=nan, num_inter_steps=K,
    ).to(device)


def _count_calls(monkeypatch):
    from py4cast_amd import _lib as L

    counts = collections.Counter()
    real = L.call

    def counting(name, *args, **kwargs):
        counts[name] += 1
        return real(name, *args, **kwargs)

    monkeypatch.setattr(L, "call", counting)
    return counts


def _train_routes(lm, case, device):
    """{mode: (prediction, loss, gradients)}: one training step per route from the same parameters."""
    from helpers import make_batch

    res = {}
    for mode, native in (("native", True), ("generic", False)):
        lm.use_native_rollout = native
        for p in lm.parameters():
            p.grad = None
        pred, _ = lm.common_step(make_batch(case, device), 0, "train")
        # K >= 2: the generic route has no fused step (its update has no loss column), the native one always carries the loss
        assert (getattr(pred, "fused_loss", None) is not None) == native, mode
        loss = lm.training_step(make_batch(case, device), 0)
        loss.backward()
        res[mode] = (pred.tensor.detach().cpu(), loss.item(), {n: p.grad.detach().cpu().clone() for n, p in lm.model.named_parameters()})
    return res


@pytest.mark.parametrize("F", [12, 21])
@pytest.mark.parametrize("nan,border", [(False, 2), (True, 0)])
def test_three_model_calls_per_target_step_equal_the_generic_path(gpu_device, F, nan, border):
    """K = 3, T = 1: three model calls, the depth the bars of tests/test_wide_rollout_gpu.py were set at.  Before the native rollout
    covered num_inter_steps >= 2 the native route was not taken here (no fused loss on either route)."""
    case = _case(seed=9, B=2, T=1, T_in=1, H=32, W=48, F=F, Ff=5, Fs=4, border=border, nan=nan)
    lm = _lm(case, 1, 1, 3, "scaled_ar", nan, gpu_device)
    lm.train()
    res = _train_routes(lm, case, gpu_device)
    a, b = res["native"], res["generic"]
    assert torch.equal(torch.isnan(a[0]), torch.isnan(b[0]))
    assert rel_err(torch.nan_to_num(a[0]), torch.nan_to_num(b[0])) < 2e-5  # BatchNorm batch statistics differ in the last bits per call
    assert abs(a[1] - b[1]) / abs(b[1]) < 1e-5
    for n in a[2]:
        assert rel_err(a[2][n], b[2][n]) < 5e-2, n  # chaotic BPTT (test_model_gpu.py); typical 1e-4


@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("nan", [False, True])
def test_deeper_schedules_without_gradients_and_their_launches(gpu_device, monkeypatch, T, nan):
    """K = 2 with T = 2 and 3 as validation_step runs them (no_grad, eval: running statistics, so both routes normalise alike)."""
    from helpers import make_batch

    K = 2
    case = _case(seed=5, B=2, T=T, T_in=1, H=32, W=48, F=12, Ff=5, Fs=4, border=0 if nan else 2, nan=nan)
    lm = _lm(case, 1, T, K, "scaled_ar", nan, gpu_device)
    lm.train()
    lm.use_native_rollout = True
    lm.training_step(make_batch(case, gpu_device), 0)   # moves the running statistics off their initial values
    lm.eval()
    counts = _count_calls(monkeypatch)
    out = {}
    with torch.no_grad():
        for mode, native in (("native", True), ("generic", False)):
            lm.use_native_rollout = native
            counts.clear()
            pred, target = lm.common_step(make_batch(case, gpu_device), 0, "val")
            fused = getattr(pred, "fused_loss", None)
            assert (fused is not None) == native
            if fused is None:
                mask, tm = lm.get_mask_on_nan(target)
                fused = lm.loss(pred, tm, mask=mask)
            out[mode] = (pred.tensor.cpu(), float(torch.mean(fused)), dict(counts))
    a, b = out["native"], out["generic"]
    assert torch.equal(torch.isnan(a[0]), torch.isnan(b[0]))
    assert rel_err(torch.nan_to_num(a[0]), torch.nan_to_num(b[0])) < 2e-5
    assert abs(a[1] - b[1]) / abs(b[1]) < 1e-5
    n = a[2]
    assert n["p4c_halfunet_forward"] == T * K
    assert sum(n.get(k, 0) for k in FREE) == T * (K - 1)
    assert n.get("p4c_ar_update_fwd", 0) == 0
    assert n["p4c_build_x"] == (T * K if nan else 1)   # the NaN-mask input channel is built by p4c_build_x per call
    assert b[2]["p4c_ar_update_fwd"] == T * K and sum(b[2].get(k, 0) for k in FREE) == 0


def test_bf16_flavour_with_two_calls_per_target_step(gpu_device):
    """bf16 maps, K = 2, T = 2, F = 60: the fused output-conv free step feeding the next call, the saved loss gradients of the loss
    steps, the free steps' adjoint on bf16 rows.  Bars of the bf16 rollout test of tests/test_wide_rollout_gpu.py."""
    from helpers import synthetic_case

    case = synthetic_case(seed=3, B=2, T=2, T_in=1, H=32, W=64, F=60, Ff=5, Fs=4, border=2)
    lm = _lm(case, 1, 2, 2, "scaled_ar", False, gpu_device, settings=BF16)
    lm.train()
    res = _train_routes(lm, case, gpu_device)
    a, b = res["native"], res["generic"]
    assert rel_err(a[0], b[0]) < 2e-2      # bf16 storage: BatchNorm statistics per call round differently
    assert abs(a[1] - b[1]) / abs(b[1]) < 1e-2
    for n in a[2]:
        x, y = a[2][n].double().flatten(), b[2][n].double().flatten()
        assert float(torch.dot(x, y) / (x.norm() * y.norm())) > 0.9, n


def test_native_rollout_with_inter_steps_is_deterministic(gpu_device):
    from helpers import make_batch, synthetic_case

    case = synthetic_case(seed=4, B=2, T=2, T_in=1, H=32, W=32, F=40, Ff=5, Fs=4, border=2)
    lm = _lm(case, 1, 2, 2, "scaled_ar", False, gpu_device)
    lm.use_native_rollout = True
    runs = []
    for _ in range(2):
        lm.load_state_dict(_lm(case, 1, 2, 2, "scaled_ar", False, gpu_device).state_dict())   # same parameters and running statistics
        lm.train()
        for p in lm.parameters():
            p.grad = None
        loss = lm.training_step(make_batch(case, gpu_device), 0)
        loss.backward()
        runs.append((loss.item(), [p.grad.detach().clone() for p in lm.model.parameters()]))
    assert runs[0][0] == runs[1][0]
    for g0, g1 in zip(runs[0][1], runs[1][1]):
        assert torch.equal(g0, g1)


@pytest.mark.parametrize("settings,bar", [(None, 2e-5), (BF16, 2e-2)], ids=["f32", "bf16"])
@pytest.mark.parametrize("strategy,K,T_in", [("scaled_ar", 1, 1), ("scaled_ar", 2, 1), ("diff_ar", 1, 1), ("diff_ar", 1, 2)])
def test_inference_forecast_equals_the_generic_path(gpu_device, monkeypatch, strategy, K, T_in, settings, bar):
    """phase "inference" (forward / predict_step): T = 4 lead times from the forcing tensor, no target, no border forcing."""
    from helpers import GRID_DIMS, feature_names, make_batch, synthetic_case
    from py4cast_amd.base import ItemBatch
    from py4cast_amd.namedtensor import NamedTensor

    T, F = 4, 12
    case = synthetic_case(seed=6, B=2, T=T, T_in=T_in, H=32, W=48, F=F, Ff=5, Fs=4, border=2)
    lm = _lm(case, T_in, T, K, strategy, False, gpu_device, settings=settings)
    lm.train()
    lm.use_native_rollout = True
    lm.training_step(make_batch(case, gpu_device), 0)   # records the names, moves the running statistics
    lm.eval()

    def batch():
        return ItemBatch(NamedTensor(case["inputs"].clone().to(gpu_device), GRID_DIMS, feature_names(F)),
                         NamedTensor(case["forcing"].clone().to(gpu_device), GRID_DIMS, [f"g{i}" for i in range(5)]), None)

    counts = _count_calls(monkeypatch)
    out = {}
    for mode, native in (("native", True), ("generic", False)):
        lm.use_native_rollout = native
        counts.clear()
        with torch.no_grad():
            pred, _ = lm.common_step(batch(), 1, "inference")
        n = dict(counts)
        unnorm = lm.predict_step(batch(), 1)
        out[mode] = (pred, n, unnorm)
    a, b = out["native"], out["generic"]
    assert a[0].tensor.shape == b[0].tensor.shape == (2, T, 32, 48, F)
    assert rel_err(a[0].tensor, b[0].tensor) < bar
    assert a[0].names == b[0].names and a[0].feature_names == b[0].feature_names and a[0].tensor.dtype == b[0].tensor.dtype
    assert getattr(a[0], "fused_loss", None) is None
    assert a[1]["p4c_halfunet_forward"] == T * K and b[1]["p4c_ar_update_fwd"] == T * K
    assert a[1].get("p4c_ar_update_fwd", 0) == 0 and sum(a[1].get(k, 0) for k in FREE) == T * K
    assert a[1]["p4c_build_x"] == (1 if T_in == 1 else T)   # a window of states is built by p4c_build_x per call
    assert rel_err(a[2].tensor, b[2].tensor) < bar
    assert a[2].names == b[2].names and a[2].feature_names == b[2].feature_names and a[2].tensor.dtype == b[2].tensor.dtype


def test_inter_steps_on_an_auto_padded_grid_stay_on_the_generic_path(gpu_device, monkeypatch):
    """H = 40 is no multiple of 16: native_rollout returns None for it, with K = 2 and for a forecast as it did for K = 1."""
    from helpers import make_batch, synthetic_case

    case = synthetic_case(seed=8, B=2, T=2, T_in=1, H=40, W=48, F=12, Ff=5, Fs=4, border=2)
    lm = _lm(case, 1, 2, 2, "scaled_ar", False, gpu_device, settings={"autopad_enabled": True})
    lm.train()
    lm.training_step(make_batch(case, gpu_device), 0)
    lm.eval()
    counts = _count_calls(monkeypatch)
    out = {}
    with torch.no_grad():
        for native in (True, False):
            lm.use_native_rollout = native
            counts.clear()
            pred, _ = lm.common_step(make_batch(case, gpu_device), 0, "val")
            assert getattr(pred, "fused_loss", None) is None
            assert counts["p4c_ar_update_fwd"] == 4 and sum(counts.get(k, 0) for k in FREE) == 0
            out[native] = pred.tensor.cpu()
    assert rel_err(out[True], out[False]) < 2e-5
