"""
Round-3 GPU tests at the BENCHMARK sizes of every BASELINE configuration: each model family is built exactly
as bench.py builds it (512 x 512 x 60 grid, the yaml widths -- hidden 1024 for UNetR++, the 6 561-node mesh for the GNNs, Swin's four
stages) and stepped through rollout + loss + backward.  The round-2 LayerNorm race (rows wider than 256 features) was invisible to
the suite because parity tests stopped at 128 features and the bench-size shapes ran only inside bench.py: these tests are where a
defect that shows only at size is caught by `pytest -m gpu`.  Also here: the generic torch-op path of Py4CastLoss.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MSE = [{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}]


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def _module(model, dtype, case, T, strategy, device, tmp):
    import bench
    from py4cast_amd.lightning import AutoRegressiveLightning

    # (UNetRPP: the published block with its conv8 channel dropout at p = 0 -- this test asserts BIT-identical reruns of the kernels)
    settings = bench.model_settings(model, dtype, unetrpp_block="published-nodrop")
    if "tmp_dir" in settings:
        settings["tmp_dir"] = tmp
    torch.manual_seed(1234)
    lm = AutoRegressiveLightning(settings, bench.make_info(case, 5), None, num_input_steps=1, num_pred_steps_train=T,
                                 num_pred_steps_val_test=T, batch_size=case["inputs"].shape[0], model_name=model, losses=MSE,
                                 training_strategy=strategy).to(device)
    return lm.train()


def _step(lm, case):
    import bench

    for p in lm.parameters():
        p.grad = None
    loss = lm.training_step(bench.make_batch(case), 0)
    loss.backward()
    torch.cuda.synchronize()
    grads = torch.cat([p.grad.detach().flatten().float() for p in lm.model.parameters() if p.grad is not None])
    return float(loss), grads


@pytest.mark.parametrize("model,T,strategy,loss_tol", [
    ("SwinUNetR", 3, "scaled_ar", 2e-2),     # BASELINE configuration 3
    ("GraphLam", 3, "scaled_ar", 2e-3),      # configuration 4 (GraphLAM: every kernel native, fixed-order reductions)
    ("HiLAM", 3, "scaled_ar", 2e-3),
    ("HiLAMParallel", 3, "scaled_ar", 2e-3),
    ("UNetRPP", 6, "diff_ar", 2e-2),         # configuration 5 (6-step diff_ar)
    ("UNet", 3, "scaled_ar", 1e-4),          # bench.py --model UNet (measured 1.1e-5: every convolution native, batch statistics)
])
def test_bench_workload_of_every_model_family(gpu_device, tmp_path_factory, model, T, strategy, loss_tol):
    """The benchmark workload of each widened model: finite prediction of the right shape, forced borders equal to the targets bit
    for bit, finite gradients for every parameter, the bf16 flavour's loss within `loss_tol` of the fp32-activation flavour's, and a
    rerun of the same step with BIT-IDENTICAL loss and gradients: every native reduction has a fixed order, and the few library
    convolutions left in SwinUNetR / UNetRPP are pinned to deterministic solvers (ops_model.library_conv2d) -- so a race or an
    uninitialised read anywhere in a step of bench size fails this test (round 2: 19 % eager-vs-eager gradient spread, all of it
    the library's atomics amplified by bf16 branch flips, profiles/r03_determinism_probe.txt)."""
    import bench

    torch.cuda.empty_cache()
    tmp = str(tmp_path_factory.mktemp("graphs"))
    case = bench.synthetic_case(1234, 2, T, 1, 512, 512, 60, 5, 4, 10, gpu_device)
    out = {}
    for dt in ("bf16", "f32"):
        lm = _module(model, dt, case, T, strategy, gpu_device, tmp)
        with torch.no_grad():
            pred, _ = lm.common_step(bench.make_batch(case), 0, "train")
        p = pred.tensor          # (graph models flatten the grid: (B, T, N, F))
        assert p.numel() == 2 * T * 512 * 512 * 60 and p.shape[:2] == (2, T) and p.shape[-1] == 60 and bool(torch.isfinite(p).all())
        if strategy == "scaled_ar":   # (lightning.py:685: only scaled_ar forces the border to the true state)
            bm = case["border_mask"][..., 0] > 0
            assert torch.equal(p.reshape(2, T, 512, 512, 60)[:, :, bm], case["outputs"][:, :, bm])   # forced border = the target
        del pred, p
        loss, g = _step(lm, case)
        assert np.isfinite(loss) and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
        if dt == "bf16":
            loss2, g2 = _step(lm, case)
            assert loss2 == loss and torch.equal(g2, g), (loss, loss2, float((g2 - g).abs().max()))
            del g2
        out[dt] = loss
        del lm, g
        torch.cuda.empty_cache()
    assert abs(out["bf16"] - out["f32"]) <= loss_tol * abs(out["f32"]), out


@pytest.mark.parametrize("name,kw", [("SmoothL1Loss", {}), ("HuberLoss", {"delta": 0.7})])
@pytest.mark.parametrize("nan", [False, True])
def test_other_torch_losses_take_the_generic_path(gpu_device, name, kw, nan):
    """py4cast/losses.py:25-31 accepts every name torch.nn has; the HIP kernels implement MSELoss / L1Loss and any other element-wise
    loss runs the reference's op sequence (losses.py:143-169, 195-210) with torch ops on the device -- values and gradients against that
    sequence written out literally in float64."""
    from helpers import make_dataset_info, synthetic_case
    from py4cast_amd.losses import NanMask, OnesMask, ScaledLoss, WeightedLoss
    from py4cast_amd.namedtensor import NamedTensor

    case = synthetic_case(seed=31, B=2, T=3, H=12, W=20, F=5, Ff=5, nan=nan)
    info = make_dataset_info(case, 5)
    names = list(info.state_weights)
    dims = ["batch", "timestep", "lat", "lon", "features"]
    tgt_raw = case["outputs"].to(gpu_device)
    pred = (torch.nan_to_num(tgt_raw) + 0.3 * torch.randn(tgt_raw.shape, generator=torch.Generator().manual_seed(5)).to(gpu_device)).requires_grad_(True)
    interior = (1.0 - case["border_mask"]).to(gpu_device)

    class LM(torch.nn.Module):
        pass

    for cls in (WeightedLoss, ScaledLoss):
        lm = LM()
        loss = cls(name, reduction="none", **kw)
        loss.prepare(lm, interior, info)
        mask = NanMask(tgt_raw) if nan else OnesMask(tgt_raw)
        target = NamedTensor(torch.nan_to_num(tgt_raw), dims, names)
        got = loss(NamedTensor(pred, dims, names), target, mask)
        got.sum().backward()
        g_got, pred.grad = pred.grad.clone(), None
        # the reference's sequence, float64
        m = (~torch.isnan(tgt_raw)).double() if nan else torch.ones_like(tgt_raw, dtype=torch.float64)
        p64 = pred.detach().double().requires_grad_(True)
        tl = getattr(torch.nn, name)(reduction="none", **kw)(p64 * m, torch.nan_to_num(tgt_raw).double() * m)
        union = torch.any(m.bool(), dim=(0, 1, 4))
        w = loss.weights(tuple(names), gpu_device).double()
        if cls is WeightedLoss:
            ref = torch.sum(torch.sum(tl * w, dim=-1) * interior[..., 0].double(), dim=(2, 3)) / (loss.num_interior - (~union).sum())
        else:
            ref = torch.sum(tl * interior.double(), dim=(2, 3)) / (loss.num_interior - (~union).sum()) * w
        ref.sum().backward()
        assert got.shape == ref.shape
        assert rel_err(got, ref) < 1e-5 and rel_err(g_got, p64.grad) < 1e-5
