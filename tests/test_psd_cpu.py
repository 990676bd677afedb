"""Power-spectrum metrics, the parts that need no GPU: the host tables, the closed form against the reference's golden spectra,
the metrics' contract (errors, keys, reset) with a numpy stand-in for the kernel, and the wiring in ``setup``."""

import os
import types

import numpy as np
import pytest
import torch

import psd_closed_form as cf

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = ["case0", "case1", "case2"]
DIMS = ["batch", "timestep", "lat", "lon", "features"]
FLAT_DIMS = ["batch", "timestep", "ngrid", "features"]


def _load(name):
    return np.load(os.path.join(GOLD, f"psd_{name}.npz"))


def test_rmax_and_bin_table_match_reference():
    from py4cast_amd import ops

    z = np.load(os.path.join(GOLD, "psd_rmax.npz"))
    assert [tuple(s) for s in z["shapes"]] == [(2, 16, 16), (2, 64, 64), (3, 24, 40), (2, 40, 24), (2, 17, 33), (1, 512, 512), (2, 512, 640)]
    assert list(z["rmax"]) == [5, 22, 11, 11, 8, 181, 249]
    for (_, H, W), rmax in zip(z["shapes"], z["rmax"]):
        assert ops.psd_rmax(int(H), int(W)) == int(rmax), (H, W)
        count = ops.psd_bin_counts(int(H), int(W))
        ref_rmax, ref_count = cf.bins(int(H), int(W))
        assert ref_rmax == int(rmax) and count.dtype == np.int32 and np.array_equal(count, ref_count) and (count > 0).all()
    for name in CASES + ["flat"]:
        z = _load(name)
        _, _, H, W, _ = z["grid_shape"]
        assert ops.psd_rmax(int(H), int(W)) == int(z["rmax"]) == z["psd_pred0"].shape[1]
    # a very elongated grid: no pixel is closer than W//2 - (H-1) to the centre, the first bins are empty (NaN in the reference)
    count = ops.psd_bin_counts(9, 64)
    assert ops.psd_rmax(9, 64) == 4 and (count == 0).all()
    assert ops.psd_rmax(1, 8) == 0


@pytest.mark.parametrize("name", CASES + ["flat"])
def test_closed_form_reproduces_reference_spectra(name):
    """the goldens carry the reference's float32 DCT (<= 6.3e-7 from float64 on white noise)"""
    z = _load(name)
    step = int(z["pred_step"])
    shape = tuple(int(v) for v in z["grid_shape"])
    for u in range(2):
        p, t, m = (torch.from_numpy(z[f"{k}{u}"]).reshape(shape) for k in ("pred", "target", "mask"))
        got = cf.spectra(p, t, m, step)
        np.testing.assert_allclose(got[0], z[f"psd_pred{u}"], rtol=1e-5, atol=0)
        np.testing.assert_allclose(got[1], z[f"psd_target{u}"], rtol=1e-5, atol=0)


def test_psd_has_no_cpu_path():
    from py4cast_amd import _lib, ops

    x = torch.zeros(1, 1, 8, 8, 2)
    with pytest.raises(_lib.P4CError):
        ops.psd(x, x, ops.MaskSpec(0), 0)
    with pytest.raises(_lib.P4CError):
        ops.psd(x.flatten(2, 3), x.flatten(2, 3), ops.MaskSpec(0), 0, grid=(8, 8))


def test_shape_errors():
    from py4cast_amd.metrics import MetricPSDK, MetricPSDVar
    from py4cast_amd.namedtensor import NamedTensor

    names = ["a", "b"]
    p = NamedTensor(torch.zeros(1, 1, 8, 8, 2), DIMS, names)
    t = NamedTensor(torch.zeros(1, 1, 8, 9, 2), DIMS, names)
    flat = NamedTensor(torch.zeros(1, 1, 64, 2), FLAT_DIMS, names)
    for metric in (MetricPSDK(None), MetricPSDVar()):
        with pytest.raises(ValueError):
            metric.update(p, t, None, None)
        with pytest.raises(ValueError):       # flattened tensors without the shape that unflattens them
            metric.update(flat, flat, None, None)
        with pytest.raises(ValueError):       # a shape that does not match the grid points
            metric.update(flat, flat, None, (1, 1, 8, 9, 2))
        assert metric.step_count == 0


@pytest.fixture
def numpy_psd(monkeypatch):
    """ops.psd replaced by the float64 closed form on the CPU: the metrics' own arithmetic and contract run without a GPU"""
    from py4cast_amd import metrics

    def psd(pred, target, spec, pred_step, grid=None):
        tgt = target
        mask = spec.tensor
        if spec.mode == 1:                      # MASK_FROM_NAN: the raw target carries the mask
            mask, tgt = ~torch.isnan(target), torch.nan_to_num(target)
        elif mask is not None and mask.dtype == torch.uint8:
            mask = mask.bool()
        return cf.spectra_torch(pred, tgt, mask, pred_step, grid)

    monkeypatch.setattr(metrics.ops, "psd", psd)
    monkeypatch.setattr(metrics, "_LAST_PSD", [None])


@pytest.mark.parametrize("name", CASES)
def test_metric_contract_keys_and_reset(name, numpy_psd, tmp_path):
    from py4cast_amd.metrics import MetricPSDK, MetricPSDVar
    from py4cast_amd.namedtensor import NamedTensor

    z = _load(name)
    step, names = int(z["pred_step"]), [str(n) for n in z["names"]]
    psdk, psdvar = MetricPSDK(tmp_path, pred_step=step), MetricPSDVar(pred_step=step)
    for u in range(2):
        p = NamedTensor(torch.from_numpy(z[f"pred{u}"]), DIMS, names)
        t = NamedTensor(torch.from_numpy(z[f"target{u}"]), DIMS, names)
        mask = torch.from_numpy(z[f"mask{u}"])
        psdk.update(p, t, mask, None)
        psdvar.update(p, t, mask, None)
        np.testing.assert_allclose(psdk.sum_psd_pred.numpy(), z[f"sum_psd_pred{u}"], rtol=1e-5)
        np.testing.assert_allclose(psdk.sum_psd_target.numpy(), z[f"sum_psd_target{u}"], rtol=1e-5)
        np.testing.assert_allclose(psdvar.sum_rmse.numpy(), z[f"sum_rmse{u}"], rtol=2e-5)
    assert psdk.step_count == 2 and psdvar.step_count == 2
    res = psdvar.compute(prefix="val")
    assert list(res) == [str(k) for k in z["rmse_keys"]] == [f"val_rmse_psd/{n}" for n in names]
    assert all(isinstance(v, torch.Tensor) and v.ndim == 0 for v in res.values())
    np.testing.assert_allclose(np.array([float(v) for v in res.values()]), z["rmse_vals"], rtol=2e-5)
    assert psdvar.step_count == 0 and psdvar.sum_rmse.ndim == 0 and psdvar.compute() == {}

    figs = psdk.compute(prefix="val")
    np.testing.assert_allclose(psdk.last_mean_psd_pred.numpy(), z["plot_pred"], rtol=1e-5)
    np.testing.assert_allclose(psdk.last_mean_psd_target.numpy(), z["plot_target"], rtol=1e-5)
    assert psdk.step_count == 0 and psdk.sum_psd_pred.ndim == 0 and psdk.sum_psd_target.ndim == 0
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        assert figs == {}
    else:
        assert list(figs) == [str(k) for k in z["psdk_keys"]] == [f"val_mean_psd_k/{n}" for n in names]
        assert all(not isinstance(f, torch.Tensor) for f in figs.values())
        for n in names:
            assert (tmp_path / "val_mean_psd_k" / f"{n}_{step + 1}.png").stat().st_size > 0
        line = figs[f"val_mean_psd_k/{names[0]}"].axes[0].lines[0]
        np.testing.assert_allclose(line.get_xdata(), z["plot_k"], rtol=1e-12)
        assert figs[f"val_mean_psd_k/{names[0]}"].axes[0].get_title() == str(z["plot_titles"][0])
    # a second epoch starts from scratch, other prefix
    p = NamedTensor(torch.from_numpy(z["pred0"]), DIMS, names)
    t = NamedTensor(torch.from_numpy(z["target0"]), DIMS, names)
    psdvar.update(p, t, None, None)
    assert sorted(psdvar.compute(prefix="test")) == sorted(f"test_rmse_psd/{n}" for n in names)


def test_flattened_input_with_shape(numpy_psd):
    """MetricPSDK of the reference on flattened tensors + shape; MetricPSDVar does the evident thing (the reference raises there);
    the caller's tensors stay flattened"""
    from py4cast_amd.metrics import MetricPSDK, MetricPSDVar
    from py4cast_amd.namedtensor import NamedTensor

    z = _load("flat")
    step, names, shape = int(z["pred_step"]), [str(n) for n in z["names"]], tuple(int(v) for v in z["grid_shape"])
    psdk, psdvar = MetricPSDK(None, pred_step=step), MetricPSDVar(pred_step=step)
    for u in range(2):
        p = NamedTensor(torch.from_numpy(z[f"pred{u}"]), FLAT_DIMS, names)
        t = NamedTensor(torch.from_numpy(z[f"target{u}"]), FLAT_DIMS, names)
        mask = torch.from_numpy(z[f"mask{u}"])
        psdk.update(p, t, mask, shape)
        psdvar.update(p, t, mask, shape)
        assert p.tensor.dim() == 4 and p.names == FLAT_DIMS and t.tensor.dim() == 4
        np.testing.assert_allclose(psdk.sum_psd_pred.numpy(), z[f"sum_psd_pred{u}"], rtol=1e-5)
        np.testing.assert_allclose(psdk.sum_psd_target.numpy(), z[f"sum_psd_target{u}"], rtol=1e-5)
    want = sum(np.sqrt(np.mean((np.log10(z[f"psd_target{u}"]) - np.log10(z[f"psd_pred{u}"])) ** 2, axis=1)) for u in range(2))
    np.testing.assert_allclose(psdvar.sum_rmse.numpy(), want, rtol=2e-5)


def test_the_two_metrics_share_one_pass(monkeypatch):
    from py4cast_amd import metrics
    from py4cast_amd.namedtensor import NamedTensor

    calls = []

    def psd(pred, target, spec, pred_step, grid=None):
        calls.append(pred_step)
        return torch.ones(2, pred.shape[-1], 3)

    monkeypatch.setattr(metrics.ops, "psd", psd)
    monkeypatch.setattr(metrics, "_LAST_PSD", [None])
    names = ["a", "b"]
    p, t = (NamedTensor(torch.zeros(1, 2, 8, 8, 2), DIMS, names) for _ in range(2))
    mask = torch.ones(1, 2, 8, 8, 2, dtype=torch.bool)
    a, b, c = metrics.MetricPSDK(None, pred_step=1), metrics.MetricPSDVar(pred_step=1), metrics.MetricPSDVar(pred_step=0)
    a.update(p, t, mask, None)
    b.update(p, t, mask, None)
    assert calls == [1]
    c.update(p, t, mask, None)             # another time step
    p.tensor.add_(1.0)                     # the same tensor object, written in place
    c.update(p, t, mask, None)
    c.update(NamedTensor(p.tensor.clone(), DIMS, names), t, mask, None)
    assert calls == [1, 0, 0, 0]


def test_setup_attaches_the_three_native_metrics(tmp_path):
    from helpers import make_dataset_info, register_test_models, synthetic_case
    from py4cast_amd.lightning import AutoRegressiveLightning
    from py4cast_amd.metrics import MetricACC, MetricPSDK, MetricPSDVar

    register_test_models()
    case = synthetic_case(H=8, W=8, F=3)
    info = make_dataset_info(case, Ff=5)
    info.shortnames.setdefault("output", [])    # MetricACC reads both lists (metrics.py:371-374 of the reference)
    lm = AutoRegressiveLightning({}, info, None, model_name="TinyConvModel", num_pred_steps_val_test=3)
    lm.trainer = types.SimpleNamespace(logger=types.SimpleNamespace(log_dir=str(tmp_path)), precision="32-true")
    with pytest.warns(UserWarning):
        lm.setup("fit")
    assert [type(m) for m in lm.list_metrics] == [MetricACC, MetricPSDK, MetricPSDVar]
    assert lm.psd_plot_metric.pred_step == 2 and lm.rmse_psd_plot_metric.pred_step == 2
    assert lm.psd_plot_metric.save_path == tmp_path
    lm.trainer = None
    lm.setup("fit")
    assert lm.list_metrics == []
