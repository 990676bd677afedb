"""GPU parity of the power-spectrum metrics (p4c_psd): against the reference's golden vectors and against the float64 closed form
(tests/psd_closed_form.py) on the two load paths and the edges.  Tolerance: the one the neighbouring rows are held to
(test_metric_acc_matches_reference)."""

import os

import numpy as np
import pytest
import torch

import psd_closed_form as cf

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DIMS = ["batch", "timestep", "lat", "lon", "features"]
FLAT_DIMS = ["batch", "timestep", "ngrid", "features"]
TOL = dict(rtol=2e-5, atol=2e-6)


def _noise(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _check(got, pred, target, mask, pred_step):
    """every grid of these tests but the one of test_empty_bins_are_nan has a pixel in every bin: all values are finite"""
    want = cf.spectra(pred, target, mask, pred_step)
    assert got.shape == want.shape and got.dtype == torch.float32 and np.isfinite(want).all()
    np.testing.assert_allclose(got.cpu().numpy(), want, **TOL)


@pytest.mark.parametrize("name", ["case0", "case1", "case2", "flat"])
def test_golden_spectra_and_metric_states(name, gpu_device):
    from py4cast_amd import ops
    from py4cast_amd.metrics import MetricPSDK, MetricPSDVar
    from py4cast_amd.namedtensor import NamedTensor

    z = np.load(os.path.join(GOLD, f"psd_{name}.npz"))
    flat = name == "flat"
    step, names = int(z["pred_step"]), [str(n) for n in z["names"]]
    shape = tuple(int(v) for v in z["grid_shape"]) if flat else None
    dims = FLAT_DIMS if flat else DIMS
    psdk, psdvar = MetricPSDK(None, pred_step=step), MetricPSDVar(pred_step=step)
    rmse = 0.0
    for u in range(2):
        p = NamedTensor(torch.from_numpy(z[f"pred{u}"]).to(gpu_device), dims, names)
        t = NamedTensor(torch.from_numpy(z[f"target{u}"]).to(gpu_device), dims, names)
        mask = torch.from_numpy(z[f"mask{u}"]).to(gpu_device)
        got = ops.psd(p.tensor, t.tensor, ops.MaskSpec.from_tensor(mask), step, grid=None if shape is None else shape[2:4])
        np.testing.assert_allclose(got[0].cpu().numpy(), z[f"psd_pred{u}"], **TOL)
        np.testing.assert_allclose(got[1].cpu().numpy(), z[f"psd_target{u}"], **TOL)
        psdk.update(p, t, mask, shape)
        psdvar.update(p, t, mask, shape)
        assert p.tensor.dim() == len(dims)
        np.testing.assert_allclose(psdk.sum_psd_pred.cpu().numpy(), z[f"sum_psd_pred{u}"], **TOL)
        np.testing.assert_allclose(psdk.sum_psd_target.cpu().numpy(), z[f"sum_psd_target{u}"], **TOL)
        if flat:    # the reference's MetricPSDVar raises on flattened input: its formula on the reference's spectra
            rmse = rmse + np.sqrt(np.mean((np.log10(z[f"psd_target{u}"]) - np.log10(z[f"psd_pred{u}"])) ** 2, axis=1))
        else:
            rmse = z[f"sum_rmse{u}"]
        np.testing.assert_allclose(psdvar.sum_rmse.cpu().numpy(), rmse, **TOL)
    res = psdvar.compute(prefix="val")
    assert list(res) == [f"val_rmse_psd/{n}" for n in names] and psdvar.step_count == 0
    if not flat:
        np.testing.assert_allclose(np.array([float(v) for v in res.values()], dtype=np.float32), z["rmse_vals"], **TOL)
    psdk.compute(prefix="val")
    np.testing.assert_allclose(psdk.last_mean_psd_pred.cpu().numpy(), z["plot_pred"], **TOL)
    np.testing.assert_allclose(psdk.last_mean_psd_target.cpu().numpy(), z["plot_target"], **TOL)
    assert psdk.step_count == 0


# (B, T, H, W, F): 16-byte path at the benchmark feature count; scalar path (F = 5, 7); H = 17 (no multiple of a slab); one sample;
# slabs of 16 and 28 rows, deep enough for the unrolled row loop and its tail (H = 780; W = 400 > H // 2 keeps every bin
# populated, see the swapped binning centre), on both paths
DEEP = (780, 400)


@pytest.mark.parametrize("shape", [(2, 1, 20, 24, 60), (2, 1, 20, 24, 5), (3, 1, 18, 31, 7), (2, 1, 17, 33, 8), (1, 1, 24, 40, 4),
                                   (1, 1, 24, 40, 3), (2, 1) + DEEP + (4,), (2, 1) + DEEP + (5,)])
def test_load_paths_and_edges_vs_closed_form(shape, gpu_device):
    from py4cast_amd import ops

    p, t = _noise(1, shape), _noise(2, shape)
    got = ops.psd(p.to(gpu_device), t.to(gpu_device), ops.MaskSpec(0), 0)
    _check(got, p, t, None, 0)


def test_batch_stride_off_16_bytes(gpu_device):
    """(B, T*H*W*F + 1) storage: sample 1 starts 4 bytes off a 16-byte boundary, the scalar loads take it as it lies"""
    from py4cast_amd import ops

    B, T, H, W, F = 2, 1, 20, 24, 8
    p, t = _noise(3, (B, T, H, W, F)), _noise(4, (B, T, H, W, F))
    views = []
    for x in (p, t):
        buf = torch.zeros(B, T * H * W * F + 1, device=gpu_device)
        v = buf[:, :-1].view(B, T, H, W, F)
        v.copy_(x)
        assert v.stride(0) % 4 == 1 and v.data_ptr() == buf.data_ptr()
        views.append(v)
    _check(ops.psd(views[0], views[1], ops.MaskSpec(0), 0), p, t, None, 0)


@pytest.mark.parametrize("pred_step", [0, 2])
def test_time_step_selection(pred_step, gpu_device):
    """the other time steps are NaN: nothing but the selected step is read"""
    from py4cast_amd import ops

    B, T, H, W, F = 2, 3, 20, 24, 8
    p, t = _noise(5, (B, T, H, W, F)), _noise(6, (B, T, H, W, F))
    for x in (p, t):
        for s in range(T):
            if s != pred_step:
                x[:, s] = float("nan")
    got = ops.psd(p.to(gpu_device), t.to(gpu_device), ops.MaskSpec(0), pred_step)
    assert torch.isfinite(got).all()
    _check(got, p, t, None, pred_step)


@pytest.mark.parametrize("F", [4, 5])
def test_mask_modes(F, gpu_device):
    from py4cast_amd import ops
    from py4cast_amd.losses import NanMask, _mask_spec
    from py4cast_amd.namedtensor import NamedTensor

    shape = (2, 2) + DEEP + (F,)
    g = torch.Generator().manual_seed(7)
    p, t = _noise(8, shape), _noise(9, shape)
    keep = torch.rand(shape, generator=g) > 0.15
    pd, td = p.to(gpu_device), t.to(gpu_device)
    # boolean mask (MASK_U8) and the same mask as floats (MASK_F32)
    u8 = ops.psd(pd, td, ops.MaskSpec.from_tensor(keep.to(gpu_device)), 1)
    _check(u8, p, t, keep, 1)
    f32 = ops.psd(pd, td, ops.MaskSpec.from_tensor(keep.float().to(gpu_device)), 1)
    assert torch.equal(u8, f32)
    # fractional float weights: the reference's fp32 product tensor * mask
    wgt = torch.rand(shape, generator=g)
    _check(ops.psd(pd, td, ops.MaskSpec.from_tensor(wgt.to(gpu_device)), 1), p, t, wgt, 1)
    # NaN marker of get_mask_on_nan (MASK_FROM_NAN) == explicit mask + nan_to_num
    raw = t.clone()
    raw[~keep] = float("nan")
    rawd = raw.to(gpu_device)
    spec, tgt = _mask_spec(NanMask(rawd), NamedTensor(rawd, DIMS, [f"f{i}" for i in range(F)]))
    assert spec.mode == 1 and tgt is rawd
    from_nan = ops.psd(pd, tgt, spec, 1)
    explicit = ops.psd(pd, torch.nan_to_num(rawd), ops.MaskSpec.from_tensor(keep.to(gpu_device)), 1)
    assert torch.equal(from_nan, explicit) and torch.equal(from_nan, u8)
    _check(from_nan, p, t, keep, 1)
    # no mask
    _check(ops.psd(pd, td, ops.MaskSpec(0), 1), p, t, None, 1)


def test_empty_bins_are_nan(gpu_device):
    """an elongated grid: the binning centre (H//2, W//2) taken as (x0, y0) lies W//2 - (H-1) = 5 rows outside a 24 x 56 grid, so
    bins 0..4 of the 11 hold no pixel -- 0/0 = NaN in the reference -- and the others hold the closed form's values"""
    from py4cast_amd import ops

    shape = (2, 1, 24, 56, 4)
    rmax, count = cf.bins(24, 56)
    assert rmax == 11 and list(count > 0) == [False] * 5 + [True] * 6
    p, t = _noise(14, shape), _noise(15, shape)
    got = ops.psd(p.to(gpu_device), t.to(gpu_device), ops.MaskSpec(0), 0).cpu().numpy()
    want = cf.spectra(p, t, None, 0)
    assert np.isnan(got[..., :5]).all() and np.isfinite(got[..., 5:]).all()
    np.testing.assert_allclose(got[..., 5:], want[..., 5:], **TOL)


def test_flattened_equals_unflattened(gpu_device):
    from py4cast_amd import ops

    shape = (2, 2, 24, 40, 8)
    p, t = _noise(10, shape).to(gpu_device), _noise(11, shape).to(gpu_device)
    keep = (torch.rand(shape, generator=torch.Generator().manual_seed(12)) > 0.1).to(gpu_device)
    a = ops.psd(p, t, ops.MaskSpec.from_tensor(keep), 1)
    b = ops.psd(p.flatten(2, 3), t.flatten(2, 3), ops.MaskSpec.from_tensor(keep.flatten(2, 3)), 1, grid=(24, 40))
    assert torch.equal(a, b)


def test_argument_errors(gpu_device):
    from py4cast_amd import _lib, ops

    x = torch.zeros(1, 1, 8, 8, 2, device=gpu_device)
    for call in (lambda: ops.psd(x, x[..., :1], ops.MaskSpec(0), 0),
                 lambda: ops.psd(x, x, ops.MaskSpec(0), 1),
                 lambda: ops.psd(x.flatten(2, 3), x.flatten(2, 3), ops.MaskSpec(0), 0),
                 lambda: ops.psd(x.flatten(2, 3), x.flatten(2, 3), ops.MaskSpec(0), 0, grid=(8, 9)),
                 lambda: ops.psd(x[:, :, :1], x[:, :, :1], ops.MaskSpec(0), 0)):         # Rmax = 0
        with pytest.raises(_lib.P4CError):
            call()


def test_full_size_properties(gpu_device):
    """At the benchmark grid: the spectra against the float64 closed form of the column sums, MetricPSDVar(x, x) == 0 exactly, and
    two calls agree bit for bit (fixed summation order, no atomics)."""
    from py4cast_amd import ops
    from py4cast_amd.metrics import MetricPSDVar
    from py4cast_amd.namedtensor import NamedTensor

    B, T, H, W, F = 1, 1, 512, 512, 60
    with torch.no_grad():
        g = torch.Generator(device="cpu").manual_seed(13)
        x, y = torch.randn(B, T, H, W, F, generator=g), torch.randn(B, T, H, W, F, generator=g)
        xd, yd = x.to(gpu_device), y.to(gpu_device)
        got = ops.psd(xd, yd, ops.MaskSpec(0), 0)
        again = ops.psd(xd, yd, ops.MaskSpec(0), 0)
        assert torch.equal(got, again)
        # closed form from the float64 column sums (the test's own O(HWF) pass, then W x 2 Rmax per feature)
        rmax, count = cf.bins(H, W)
        assert got.shape == (2, F, rmax) and (count > 0).all()
        h, w, k = np.arange(H), np.arange(W), np.arange(2 * rmax)
        col = torch.from_numpy(np.cos(np.pi * (2 * h + 1) * (H - 1) / (2 * H)))
        basis = np.cos(np.pi * np.outer(2 * w + 1, k) / (2 * W)) * np.where(k == 0, np.sqrt(1.0 / W), np.sqrt(2.0 / W)) / np.sqrt(H)
        last = np.cos(np.pi * (2 * w + 1) * (W - 1) / (2 * W)) * np.sqrt(2.0 / H) * np.sqrt(2.0 / W)
        q = np.arange(rmax)
        for i, t in enumerate((x, y)):
            td = t[0, 0].double()                                               # (H, W, F)
            s0, s1 = td.sum(0).numpy(), torch.einsum("h,hwf->wf", col, td).numpy()
            sig = (s0.T @ basis) ** 2 / W ** 2                                  # (F, 2 Rmax), B = 1
            sig_last = (s1.T @ last) ** 2 / W ** 2                              # (F,)
            left = np.where(q[None, :] == 0, sig_last[:, None], sig[:, np.maximum(2 * q - 1, 0)])
            want = sig[:, 2 * q] + 0.5 * left + 0.5 * sig[:, 2 * q + 1]
            np.testing.assert_allclose(got[i].cpu().numpy(), want, rtol=2e-5, atol=0)
        names = [f"f{j}" for j in range(F)]
        m = MetricPSDVar(pred_step=0)
        m.update(NamedTensor(xd, DIMS, names), NamedTensor(xd, DIMS, names), None, None)
        assert m.sum_rmse.shape == (F,) and torch.equal(m.sum_rmse, torch.zeros_like(m.sum_rmse))


def test_validation_epoch_logs_psd_scalars(gpu_device, tmp_path):
    """setup -> validation_step -> on_validation_epoch_end with a logger: the native pair is notified next to MetricACC and the
    epoch logs val_rmse_psd/* (tensors) and hands val_mean_psd_k/* (figures) on -- no py4cast package involved"""
    import types

    from helpers import make_batch, make_dataset_info, register_test_models, synthetic_case
    from py4cast_amd.lightning import AutoRegressiveLightning

    register_test_models()
    case = synthetic_case(seed=3, B=2, T=3, H=16, W=24, F=3)
    info = make_dataset_info(case, Ff=5)
    info.shortnames.setdefault("output", [])
    lm = AutoRegressiveLightning({}, info, None, num_input_steps=1, num_pred_steps_train=3, num_pred_steps_val_test=3, batch_size=2,
                                 model_name="TinyConvModel").to(gpu_device)
    lm.trainer = types.SimpleNamespace(logger=types.SimpleNamespace(log_dir=str(tmp_path)), precision="32-true")
    logged = {}
    lm.log_dict = lambda d, **kw: logged.update(d)
    with pytest.warns(UserWarning):
        lm.setup("fit")
    lm.on_validation_start()
    lm.validation_step(make_batch(case, gpu_device), 0)
    assert lm.psd_plot_metric.step_count == 1 and lm.rmse_psd_plot_metric.step_count == 1
    lm.on_validation_epoch_end()
    names = info.shortnames["input_output"]
    assert all(f"val_rmse_psd/{n}" in logged for n in names)
    with torch.no_grad():
        pred, target = lm.common_step(make_batch(case, gpu_device), 0, phase="val_test")
    want = cf.spectra(pred.tensor.cpu(), target.tensor.cpu(), None, 2)
    rmse = np.sqrt(np.mean((np.log10(want[1]) - np.log10(want[0])) ** 2, axis=1))
    np.testing.assert_allclose([float(logged[f"val_rmse_psd/{n}"]) for n in names], rmse, **TOL)
    np.testing.assert_allclose(lm.psd_plot_metric.last_mean_psd_pred.cpu().numpy(), want[0], **TOL)
    assert lm.psd_plot_metric.step_count == 0
