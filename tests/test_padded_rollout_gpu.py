"""
The native HalfUNet rollout on auto-padded grids (``autopad_enabled``, a grid that is not a multiple of 16; one input state, one model
call per target step): the network side on the padded grid, the state side untouched at H x W, connected by the window kernels of
csrc/rollout_win.hip.  Checked against the generic per-op route on the same parameters (``lm.use_native_rollout = False``: forward pads
and crops around the plan) with the bars of tests/test_inter_steps_rollout_gpu.py, against the float64 oracle rollout around
pad -> oracle/halfunet.py -> crop with the method of tests/test_model_gpu.py, and by counting each route's launches (``_lib.call``).
Grids: 33 x 47 -> 48 x 48 (top 7, bottom 8, left 0, right 1) and 40 x 72 -> 48 x 80 (4 each side).
"""
import collections
import copy

import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

BF16 = {"compute_dtype": "bf16", "activation_dtype": "bf16"}
GRIDS = [(33, 47), (40, 72)]
WIN = ("p4c_build_x_win", "p4c_ar_update_loss_fwd_win", "p4c_ar_update_next_win", "p4c_ar_update_loss_bwd_win")
RATIO = 1.5   # tests/test_halfunet_settings_bf16_gpu.py
GPRED = 0.3   # tests/rollout_nodes.py


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _case(nan=False, **kw):
    """helpers.synthetic_case with the NaNs of tests/test_inter_steps_rollout_gpu.py planted for any T"""
    from helpers import synthetic_case

    case = synthetic_case(nan=False, **kw)
    if nan:
        case["inputs"][0, 0, 3, 4, 1] = float("nan")
        case["forcing"][-1, -1, 5, 6, 2] = float("nan")
        case["outputs"][:, :, 7, 8, :] = float("nan")
        case["outputs"][0, -1, 2, 2, 0] = float("nan")
    return case


def _lm(case, T_in, T, K, strategy, nan, device, settings=None, weight=0.7, autopad=True):
    from helpers import make_dataset_info
    from py4cast_amd.lightning import AutoRegressiveLightning

    info = make_dataset_info(case, case["forcing"].shape[-1])
    torch.manual_seed(0)
    return AutoRegressiveLightning(
        dict(settings or {}, autopad_enabled=autopad), info, None, num_input_steps=T_in, num_pred_steps_train=T, batch_size=2,
        model_name="HalfUNet", losses=[{"class": "WeightedLoss", "weight": weight, "params": {"loss": "MSELoss", "reduction": "none"}}],
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


def _train_routes(lm, case, device, counts=None, gpred=None):
    """{mode: (prediction, loss, gradients, launches of the training step)}: one training step per route from the same parameters"""
    from helpers import make_batch

    res = {}
    for mode, native in (("native", True), ("generic", False)):
        lm.use_native_rollout = native
        for p in lm.parameters():
            p.grad = None
        if counts is not None:
            counts.clear()
        if gpred is None:
            pred, _ = lm.common_step(make_batch(case, device), 0, "train")
            pred = pred.tensor
            if counts is not None:
                counts.clear()
            loss = lm.training_step(make_batch(case, device), 0)
        else:   # somebody differentiates through the prediction itself
            # (the generic route's fused step writes the prediction into a plain buffer: only its unfused form carries g_pred)
            lm.use_fused_step = native
            pred, target = lm.common_step(make_batch(case, device), 0, "train")
            fused = getattr(pred, "fused_loss", None)
            if fused is None:
                mask, tm = lm.get_mask_on_nan(target)
                fused = lm.loss(pred, tm, mask=mask)
            pred = pred.tensor
            loss = torch.mean(fused) + GPRED * (pred * gpred.to(device)).sum()
        loss.backward()
        res[mode] = (pred.detach().cpu(), loss.item(), {n: p.grad.detach().cpu().clone() for n, p in lm.model.named_parameters()},
                     dict(counts) if counts is not None else None)
    return res


def _assert_f32(a, b):
    assert torch.equal(torch.isnan(a[0]), torch.isnan(b[0]))
    assert rel_err(torch.nan_to_num(a[0]), torch.nan_to_num(b[0])) < 2e-5  # BatchNorm batch statistics differ in the last bits per call
    assert abs(a[1] - b[1]) / abs(b[1]) < 1e-5
    for n in a[2]:
        assert rel_err(a[2][n], b[2][n]) < 5e-2, n  # chaotic BPTT (test_model_gpu.py); typical 1e-4


def _assert_bf16(a, b):
    assert torch.equal(torch.isnan(a[0]), torch.isnan(b[0]))
    assert rel_err(torch.nan_to_num(a[0]), torch.nan_to_num(b[0])) < 2e-2      # bf16 storage: BatchNorm statistics per call round differently
    assert abs(a[1] - b[1]) / abs(b[1]) < 1e-2
    for n in a[2]:
        x, y = a[2][n].double().flatten(), b[2][n].double().flatten()
        assert float(torch.dot(x, y) / (x.norm() * y.norm())) > 0.9, n


def _assert_launches(native, generic, T):
    """THE test of the route: on the parent commit a padded grid never reached the native rollout"""
    for name in ("p4c_build_x_win", "p4c_ar_update_loss_fwd_win", "p4c_ar_update_loss_bwd_win", "p4c_halfunet_forward"):
        assert native.get(name, 0) == T, (name, native)
    for name in ("p4c_build_x", "p4c_ar_update_fwd", "p4c_ar_update_loss_fwd", "p4c_ar_update_next_win"):
        assert native.get(name, 0) == 0, (name, native)
    assert all(generic.get(name, 0) == 0 for name in WIN), generic


@pytest.mark.parametrize("strategy", ["scaled_ar", "diff_ar"])
@pytest.mark.parametrize("nan,border", [(False, 2), (True, 0)])
@pytest.mark.parametrize("F", [12, 21])
@pytest.mark.parametrize("H,W", GRIDS)
@pytest.mark.parametrize("settings", [None, BF16], ids=["f32", "bf16"])
def test_training_on_a_padded_grid_equals_the_generic_path(gpu_device, monkeypatch, settings, H, W, F, nan, border, strategy):
    T = 2
    case = _case(seed=9, B=2, T=T, T_in=1, H=H, W=W, F=F, Ff=5, Fs=4, border=border, nan=nan)
    lm = _lm(case, 1, T, 1, strategy, nan, gpu_device, settings=settings)
    lm.train()
    res = _train_routes(lm, case, gpu_device, counts=_count_calls(monkeypatch))
    _assert_launches(res["native"][3], res["generic"][3], T)
    (_assert_bf16 if settings else _assert_f32)(res["native"], res["generic"])
    assert all(int(b) > 0 for n, b in lm.model.named_buffers() if n.endswith("num_batches_tracked"))


@pytest.mark.parametrize("H,W", GRIDS)
@pytest.mark.parametrize("settings,pbar,lbar", [(None, 2e-5, 1e-5), (BF16, 2e-2, 1e-2)], ids=["f32", "bf16"])
def test_validation_on_a_padded_grid(gpu_device, monkeypatch, settings, pbar, lbar, H, W):
    """eval mode under no_grad, as validation_step runs it (running statistics: both routes normalise alike)"""
    from helpers import make_batch

    T = 2
    case = _case(seed=5, B=2, T=T, T_in=1, H=H, W=W, F=12, Ff=5, Fs=4, border=2)
    lm = _lm(case, 1, T, 1, "scaled_ar", False, gpu_device, settings=settings)
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
            fused = getattr(pred, "fused_loss", None)   # (K = 1: the generic route carries a fused step's loss too)
            assert fused is not None or not native
            if fused is None:
                mask, tm = lm.get_mask_on_nan(target)
                fused = lm.loss(pred, tm, mask=mask)
            out[mode] = (pred.tensor.cpu(), float(torch.mean(fused)), dict(counts))
    a, b = out["native"], out["generic"]
    assert rel_err(a[0], b[0]) < pbar
    assert abs(a[1] - b[1]) / abs(b[1]) < lbar
    assert a[2]["p4c_build_x_win"] == T and a[2]["p4c_ar_update_loss_fwd_win"] == T and a[2].get("p4c_ar_update_loss_bwd_win", 0) == 0
    assert all(b[2].get(name, 0) == 0 for name in WIN)


@pytest.mark.parametrize("H,W,strategy", [(33, 47, "scaled_ar"), (40, 72, "diff_ar")])
@pytest.mark.parametrize("settings,bar", [(None, 2e-5), (BF16, 2e-2)], ids=["f32", "bf16"])
def test_inference_forecast_on_a_padded_grid(gpu_device, monkeypatch, settings, bar, H, W, strategy):
    """phase "inference" (forward / predict_step): T = 3 lead times from the forcing tensor, no target, no border forcing"""
    from helpers import GRID_DIMS, feature_names, make_batch
    from py4cast_amd.base import ItemBatch
    from py4cast_amd.namedtensor import NamedTensor

    T, F = 3, 12
    case = _case(seed=6, B=2, T=T, T_in=1, H=H, W=W, F=F, Ff=5, Fs=4, border=2)
    lm = _lm(case, 1, T, 1, strategy, False, gpu_device, settings=settings)
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
    assert a[0].tensor.shape == b[0].tensor.shape == (2, T, H, W, F)
    assert rel_err(a[0].tensor, b[0].tensor) < bar
    assert a[0].names == b[0].names and a[0].feature_names == b[0].feature_names and a[0].tensor.dtype == b[0].tensor.dtype
    assert getattr(a[0], "fused_loss", None) is None
    assert a[1]["p4c_ar_update_next_win"] == T and a[1]["p4c_build_x_win"] == T and a[1]["p4c_halfunet_forward"] == T
    assert a[1].get("p4c_ar_update_fwd", 0) == 0 and a[1].get("p4c_build_x", 0) == 0 and a[1].get("p4c_ar_update_next", 0) == 0
    assert b[1]["p4c_ar_update_fwd"] == T and all(b[1].get(name, 0) == 0 for name in WIN)
    assert rel_err(a[2].tensor, b[2].tensor) < bar
    assert a[2].names == b[2].names and a[2].feature_names == b[2].feature_names and a[2].tensor.dtype == b[2].tensor.dtype
    assert a[2].tensor.shape == b[2].tensor.shape


def _oracle(case, ref, dt, H, W, T):
    """loss and parameter gradients of the oracle rollout around pad -> ref -> crop in ``dt``"""
    from oracle import losses as olosses
    from oracle import rollout as orollout
    from padded_rollout_reference import padding_for

    top, bottom, left, right = padding_for(H, W)
    c = {k: v.to(dt) for k, v in case.items()}
    statics = c["statics"].unsqueeze(0).expand(2, *c["statics"].shape)
    interior = 1.0 - c["border_mask"]
    ref.train()

    def model(x):
        return ref(Fn.pad(x, (left, right, top, bottom)))[:, :, top:top + H, left:left + W]

    pred = orollout.rollout(model, c["inputs"], c["forcing"], c["outputs"], statics, c["border_mask"], interior, c["diff_std"], c["diff_mean"],
                            "scaled_ar", 1, False, "train", features_second=True)
    wts = olosses.weighted_loss_weights(c["state_weight"], c["diff_std"], "mse")
    loss = olosses.training_loss(pred, c["outputs"], False, [("WeightedLoss", 1.0, dict(weights=wts, interior_mask=interior, kind="mse"))])
    loss.backward()
    return loss, dict(ref.named_parameters()), pred.detach()


def test_padded_training_step_matches_the_float64_oracle(gpu_device):
    """fp32 flavour, 33 x 47, T = 2: loss and BPTT gradients against the float64 oracle rollout with pad -> HalfUNetRef -> crop, by the
    method and _noise_bar of tests/test_model_gpu.py::test_training_step_with_halfunet_matches_oracle (floor of its T = 3 case: the
    gradient passes through more than one randomly initialised network)."""
    from helpers import make_batch
    from oracle.halfunet import HalfUNetRef
    from test_model_gpu import _noise_bar

    H, W, T = 33, 47, 2
    case = _case(seed=5, B=2, T=T, T_in=1, H=H, W=W, F=12, Ff=5, Fs=4, border=2)
    lm = _lm(case, 1, T, 1, "scaled_ar", False, "cpu", weight=1.0)
    ref32 = HalfUNetRef(12 + 4 + 5, 12)
    ref32.load_state_dict(lm.model.state_dict())
    ref64 = copy.deepcopy(ref32).double()
    lm = lm.to(gpu_device)
    lm.train()
    lm.use_native_rollout = True
    pred, _ = lm.common_step(make_batch(case, gpu_device), 0, "train")
    assert getattr(pred, "fused_loss", None) is not None
    for p in lm.parameters():
        p.grad = None
    loss = lm.training_step(make_batch(case, gpu_device), 0)
    loss.backward()
    l64, p64, _ = _oracle(case, ref64, torch.float64, H, W, T)
    l32, p32, _ = _oracle(case, ref32, torch.float32, H, W, T)
    print(f"padded oracle: loss {abs(loss.item() - l64.item()) / abs(l64.item()):.3e}")
    assert abs(loss.item() - l64.item()) / abs(l64.item()) < 1e-4
    for name, p in lm.model.named_parameters():
        err, noise = rel_err(p.grad, p64[name].grad), rel_err(p32[name].grad, p64[name].grad)
        print(f"padded oracle: {name} {err:.3e} (torch fp32 on the CPU: {noise:.3e})")
        assert err < _noise_bar(noise, 6e-2), name


def test_bf16_padded_training_step_is_as_close_to_float64_as_the_generic_route(gpu_device):
    """bf16 flavour, 33 x 47, T = 2: the native route's distance from the float64 oracle (pad -> HalfUNetRef -> crop) is at most RATIO
    times the generic route's on the same case: for the loss, and for the prediction and the gradient as a whole (relative L2 over
    all elements).
    Measured on an MI355X: loss 3.5372e-05 on both routes, gradient 2.8207e-01 on both, prediction 1.3392e-02 on both -- the two
    routes hand the plan the same padded input bits and the window kernels equal the dense ones, so they agree to every printed digit."""
    from helpers import make_batch
    from oracle.halfunet import HalfUNetRef

    H, W, T = 33, 47, 2
    case = _case(seed=5, B=2, T=T, T_in=1, H=H, W=W, F=12, Ff=5, Fs=4, border=2)
    lm = _lm(case, 1, T, 1, "scaled_ar", False, "cpu", settings=BF16, weight=1.0)
    ref64 = HalfUNetRef(12 + 4 + 5, 12)
    ref64.load_state_dict(lm.model.state_dict())
    ref64 = ref64.double()
    lm = lm.to(gpu_device)
    lm.train()
    l64, p64, pred64 = _oracle(case, ref64, torch.float64, H, W, T)
    want = torch.cat([p64[n].grad.flatten() for n, _ in lm.model.named_parameters()])
    dist = {}
    for mode, native in (("native", True), ("generic", False)):
        lm.use_native_rollout = native
        for p in lm.parameters():
            p.grad = None
        pred, _ = lm.common_step(make_batch(case, gpu_device), 0, "train")
        pred = pred.tensor.detach().cpu().double()
        loss = lm.training_step(make_batch(case, gpu_device), 0)
        loss.backward()
        got = torch.cat([p.grad.detach().cpu().double().flatten() for _, p in lm.model.named_parameters()])
        dist[mode] = (abs(loss.item() - l64.item()) / abs(l64.item()), float((got - want).norm() / want.norm()),
                      float((pred - pred64).norm() / pred64.norm()))
    n, g = dist["native"], dist["generic"]
    print(f"padded bf16 vs float64: loss native {n[0]:.4e} generic {g[0]:.4e}; gradient native {n[1]:.4e} generic {g[1]:.4e}; "
          f"prediction native {n[2]:.4e} generic {g[2]:.4e}")
    assert n[0] <= RATIO * g[0]
    assert n[1] <= RATIO * g[1]
    assert n[2] <= RATIO * g[2]


def test_padded_native_rollout_is_deterministic(gpu_device):
    from helpers import make_batch

    case = _case(seed=4, B=2, T=2, T_in=1, H=33, W=47, F=20, Ff=5, Fs=4, border=2)
    lm = _lm(case, 1, 2, 1, "scaled_ar", False, gpu_device)
    lm.use_native_rollout = True
    runs = []
    for _ in range(2):
        lm.load_state_dict(_lm(case, 1, 2, 1, "scaled_ar", False, gpu_device).state_dict())   # same parameters and running statistics
        lm.train()
        for p in lm.parameters():
            p.grad = None
        loss = lm.training_step(make_batch(case, gpu_device), 0)
        loss.backward()
        runs.append((loss.item(), [p.grad.detach().clone() for p in lm.model.parameters()]))
    assert runs[0][0] == runs[1][0]
    for g0, g1 in zip(runs[0][1], runs[1][1]):
        assert torch.equal(g0, g1)


def test_gradient_through_the_prediction_on_a_padded_grid(gpu_device, monkeypatch):
    """loss + GPRED * (prediction * R).sum(), as the gpred cases of tests/rollout_nodes.py: g_pred is state-sided and dense"""
    T, F, H, W = 2, 12, 33, 47
    case = _case(seed=9, B=2, T=T, T_in=1, H=H, W=W, F=F, Ff=5, Fs=4, border=2)
    lm = _lm(case, 1, T, 1, "scaled_ar", False, gpu_device)
    lm.train()
    R = torch.randn(2, T, H, W, F, generator=torch.Generator().manual_seed(109))
    counts = _count_calls(monkeypatch)
    res = _train_routes(lm, case, gpu_device, counts=counts, gpred=R)
    assert res["native"][3]["p4c_ar_update_loss_bwd_win"] == T
    _assert_f32(res["native"], res["generic"])


@pytest.mark.parametrize("what", ["K=2", "T_in=2", "fits"])
def test_other_configurations_launch_no_window_kernel(gpu_device, monkeypatch, what):
    """padded grids with num_inter_steps >= 2 or num_input_steps >= 2 stay on the generic route; a grid that fits stays on the dense
    native route"""
    from helpers import make_batch

    K, T_in = (2 if what == "K=2" else 1), (2 if what == "T_in=2" else 1)
    H, W = (32, 48) if what == "fits" else (33, 47)
    case = _case(seed=8, B=2, T=2, T_in=T_in, H=H, W=W, F=12, Ff=5, Fs=4, border=2)
    lm = _lm(case, T_in, 2, K, "scaled_ar", False, gpu_device)
    lm.train()
    counts = _count_calls(monkeypatch)
    loss = lm.training_step(make_batch(case, gpu_device), 0)
    loss.backward()
    assert all(counts.get(name, 0) == 0 for name in WIN), dict(counts)
    assert counts["p4c_halfunet_forward"] == 2 * K
    if what == "fits":
        assert counts["p4c_build_x"] >= 1 and counts.get("p4c_ar_update_fwd", 0) == 0    # the dense native route
    else:
        assert counts["p4c_ar_update_fwd"] + counts.get("p4c_ar_update_loss_fwd", 0) == 2 * K   # the generic route
    with torch.no_grad():
        lm.eval()
        counts.clear()
        from helpers import GRID_DIMS, feature_names
        from py4cast_amd.base import ItemBatch
        from py4cast_amd.namedtensor import NamedTensor

        batch = ItemBatch(NamedTensor(case["inputs"].clone().to(gpu_device), GRID_DIMS, feature_names(12)),
                          NamedTensor(case["forcing"].clone().to(gpu_device), GRID_DIMS, [f"g{i}" for i in range(5)]), None)
        lm.common_step(batch, 1, "inference")
        assert all(counts.get(name, 0) == 0 for name in WIN), dict(counts)


def test_a_padded_grid_without_autopad_still_raises(gpu_device, monkeypatch):
    from helpers import make_batch

    case = _case(seed=8, B=2, T=2, T_in=1, H=33, W=47, F=12, Ff=5, Fs=4, border=2)
    lm = _lm(case, 1, 2, 1, "scaled_ar", False, gpu_device, autopad=False)
    lm.train()
    counts = _count_calls(monkeypatch)
    with pytest.raises(Exception, match="multiple of 16"):
        lm.training_step(make_batch(case, gpu_device), 0)
    assert all(counts.get(name, 0) == 0 for name in WIN)
