"""
The one-node native rollout with num_input_steps = T_in >= 2 (HalfUNetMI355X.native_rollout): step i's input is the window of
states i .. i+T_in-1 of a (T_in + T)-slot buffer, and the reverse sweep sums each state's gradient in HIP (p4c_sum_state_grads).
Checked against the generic per-op autograd path on the same kernels, as tests/test_model_gpu.py does for T_in = 1.
The float64 check of this rollout, call by call and past the wrap of the gradient ring, is tests/test_rollout_nodes_gpu.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _lm(case, T_in, T, strategy, nan, device, settings=None, weight=0.7):
    from helpers import make_dataset_info
    from py4cast_amd.lightning import AutoRegressiveLightning

    info = make_dataset_info(case, case["forcing"].shape[-1])
    torch.manual_seed(0)
    return AutoRegressiveLightning(
        settings or {}, info, None, num_input_steps=T_in, num_pred_steps_train=T, batch_size=2, model_name="HalfUNet",
        losses=[{"class": "WeightedLoss", "weight": weight, "params": {"loss": "MSELoss", "reduction": "none"}}],
        training_strategy=strategy, mask_on_nan=nan,
    ).to(device)


def _routes(lm, case, device):
    from helpers import make_batch

    res = {}
    for mode, native, fused in (("native", True, True), ("generic_fused", False, True), ("generic", False, False)):
        lm.use_native_rollout, lm.use_fused_step = native, fused
        for p in lm.parameters():
            p.grad = None
        pred, _ = lm.common_step(make_batch(case, device), 0, "train")
        assert (getattr(pred, "fused_loss", None) is not None) == (native or fused), mode
        loss = lm.training_step(make_batch(case, device), 0)
        loss.backward()
        res[mode] = (pred.tensor.detach().cpu(), loss.item(), {n: p.grad.detach().cpu().clone() for n, p in lm.model.named_parameters()})
    return res


@pytest.mark.parametrize("T_in,F", [(2, 12), (3, 12), (2, 40)])
@pytest.mark.parametrize("strategy,nan,border", [("scaled_ar", False, 2), ("scaled_ar", True, 0), ("diff_ar", False, 0)])
def test_native_rollout_with_input_window_equals_generic_path(gpu_device, T_in, F, strategy, nan, border):
    """(2, 40): 89 input channels, the gradient of state channels 64 .. 79 crosses a data-gradient block boundary."""
    from helpers import synthetic_case

    case = synthetic_case(seed=9, B=2, T=3, T_in=T_in, H=32, W=48, F=F, Ff=5, Fs=4, border=border, nan=nan)
    lm = _lm(case, T_in, 3, strategy, nan, gpu_device)
    lm.train()
    res = _routes(lm, case, gpu_device)
    for mode in ("native", "generic_fused"):
        a, b = res[mode][0], res["generic"][0]
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert rel_err(torch.nan_to_num(a), torch.nan_to_num(b)) < 2e-5  # BatchNorm batch statistics differ in the last bits per call
        assert abs(res[mode][1] - res["generic"][1]) / abs(res["generic"][1]) < 1e-5
        for n in res[mode][2]:
            assert rel_err(res[mode][2][n], res["generic"][2][n]) < 5e-2, (mode, n)  # chaotic BPTT (test_model_gpu.py); typical 1e-4


def test_native_rollout_with_input_window_bf16_wide(gpu_device):
    """bf16 flavour at F = 60, T_in = 2: 129 input channels (the K-chunked first convolution), the fused output-conv + update + loss
    step without "feed next step", the saved loss gradients, three data-gradient blocks."""
    from helpers import synthetic_case

    case = synthetic_case(seed=3, B=2, T=3, T_in=2, H=32, W=64, F=60, Ff=5, Fs=4, border=2)
    lm = _lm(case, 2, 3, "scaled_ar", False, gpu_device, settings={"compute_dtype": "bf16", "activation_dtype": "bf16"})
    lm.train()
    res = _routes(lm, case, gpu_device)
    a, b = res["native"], res["generic_fused"]
    assert rel_err(a[0], b[0]) < 2e-2      # bf16 storage: BatchNorm statistics per call round differently
    assert abs(a[1] - b[1]) / abs(b[1]) < 1e-2
    for n in a[2]:
        x, y = a[2][n].double().flatten(), b[2][n].double().flatten()
        assert float(torch.dot(x, y) / (x.norm() * y.norm())) > 0.9, n


def test_native_rollout_with_input_window_is_deterministic(gpu_device):
    from helpers import make_batch, synthetic_case

    case = synthetic_case(seed=4, B=2, T=3, T_in=2, H=32, W=32, F=40, Ff=5, Fs=4, border=2)
    lm = _lm(case, 2, 3, "scaled_ar", False, gpu_device)
    lm.use_native_rollout = True
    runs = []
    for _ in range(2):
        lm.load_state_dict(_lm(case, 2, 3, "scaled_ar", False, gpu_device).state_dict())   # same parameters and running statistics
        lm.train()
        for p in lm.parameters():
            p.grad = None
        loss = lm.training_step(make_batch(case, gpu_device), 0)
        loss.backward()
        runs.append((loss.item(), [p.grad.detach().clone() for p in lm.model.parameters()]))
    assert runs[0][0] == runs[1][0]
    for g0, g1 in zip(runs[0][1], runs[1][1]):
        assert torch.equal(g0, g1)


def test_native_rollout_with_input_window_accumulates_into_flat_grad_buffer(gpu_device):
    from helpers import make_batch, synthetic_case
    from py4cast_amd.trainer import FlatDDP

    case = synthetic_case(seed=4, B=2, T=2, T_in=2, H=32, W=32, F=12, Ff=5, Fs=4, border=0, nan=False)
    lm = _lm(case, 2, 2, "scaled_ar", False, gpu_device, weight=1.0)
    lm.train()
    lm.use_native_rollout = True
    for p in lm.parameters():
        p.grad = None
    lm.training_step(make_batch(case, gpu_device), 0).backward()
    ref = {n: p.grad.detach().clone() for n, p in lm.model.named_parameters()}
    ddp = FlatDDP(lm, world_size=1)
    assert lm.model._flat_grad_target() is not None
    for k in (1, 2):
        lm.training_step(make_batch(case, gpu_device), 0).backward()
        for n, p in lm.model.named_parameters():
            assert rel_err(p.grad, k * ref[n]) < 5e-2, (k, n)  # BatchNorm running stats move between calls; typical 1e-4
    assert float(ddp.flat_grad.abs().sum()) > 0
