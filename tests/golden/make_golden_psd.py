#!/usr/bin/env python3
"""
Golden vectors for the power-spectrum validation metrics -- runs ONLY in the build container (needs the reference and scipy).

Executes the reference's unmodified ``py4cast/metrics.py`` (``power_spectral_density``, ``MetricPSDK``, ``MetricPSDVar``,
lines 13-352) on seeded white noise through the ``sys.modules`` stubs of ``make_golden_next.py`` and stores, per case, the
inputs, the spectra of prediction and target, the two metrics' states after each of two ``update`` calls and what ``compute``
returns.  ``plot_log_psd`` is a stub that draws nothing and records the arrays it is handed.

White noise has a flat spectrum, which keeps ``log10`` well conditioned.  The time steps a case does not select hold small
integers (they compress to almost nothing; a kernel that picked the wrong step would still miss every value).

    python tests/golden/make_golden_psd.py
"""

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (stub helpers, NamedTensor shim)

DIMS = ["batch", "timestep", "lat", "lon", "features"]


class NT(mg.NamedTensor):
    def unflatten_(self, dim, unflattened_size, unflatten_dim_name):
        self.tensor = self.tensor.unflatten(dim, unflattened_size)
        self.names = self.names[:dim] + list(unflatten_dim_name) + self.names[dim + 1:]


class Metric(torch.nn.Module):  # torchmetrics.Metric: state registry only
    def __init__(self):
        super().__init__()
        self._defaults = {}

    device = property(lambda s: torch.device("cpu"))

    def add_state(self, name, default, dist_reduce_fx=None):
        self._defaults[name] = default.clone()
        setattr(self, name, default.clone())

    def reset(self):
        for k, v in self._defaults.items():
            setattr(self, k, v.clone())


class FakeFigure:
    def savefig(self, *a, **k):
        raise AssertionError("the save path of the generator does not exist")


PLOTTED = []


def plot_log_psd(k, psd_pred, psd_target, title):
    PLOTTED.append((np.array(k), np.array(psd_pred), np.array(psd_target), title))
    return FakeFigure()


def load_reference():
    mg.stub("torchmetrics", Metric=Metric)
    mg.stub("py4cast.datasets", get_datasets=None)
    mg.stub("py4cast.datasets.base", DatasetInfo=object, NamedTensor=NT)
    mg.stub("py4cast.plots", plot_log_psd=plot_log_psd)
    sys.path.insert(0, mg.REF)
    return importlib.import_module("py4cast.metrics")  # unmodified reference file


def noise(g, shape, pred_step):
    x = torch.randint(-2, 3, shape, generator=g).float()
    x[:, pred_step] = torch.randn(shape[:1] + shape[2:], generator=g)
    return x


def spectrum(metrics, x, mask, pred_step):
    """power_spectral_density on (B, F, H, W) of tensor * mask, as MetricPSDK.add_psd slices it (metrics.py:121-144)"""
    xm = (x * mask).permute(0, -1, 2, 3, 1)[..., pred_step]
    return metrics.power_spectral_density(xm.numpy())


def gen_case(metrics, name, seed, shape, pred_step, flat=False):
    from pathlib import Path

    g = torch.Generator().manual_seed(seed)
    B, T, H, W, F = shape
    names = [f"f{i}" for i in range(F)]
    psdk = metrics.MetricPSDK(Path("/nonexistent/psd_golden"), pred_step=pred_step)
    psdvar = None if flat else metrics.MetricPSDVar(pred_step=pred_step)   # the reference's MetricPSDVar raises on flattened input
    out = {"pred_step": np.int64(pred_step), "names": np.array(names), "grid_shape": np.array(shape, dtype=np.int64)}
    for step in range(2):
        p, t = noise(g, shape, pred_step), noise(g, shape, pred_step)
        mask = (torch.rand(shape, generator=g) > 0.1) if step == 1 else torch.ones(shape, dtype=torch.bool)
        out[f"psd_pred{step}"] = spectrum(metrics, p, mask, pred_step)
        out[f"psd_target{step}"] = spectrum(metrics, t, mask, pred_step)
        if flat:
            pf, tf, mf = p.flatten(2, 3), t.flatten(2, 3), mask.flatten(2, 3)
            pn, tn = NT(pf, DIMS[:2] + ["ngrid", "features"], names), NT(tf, DIMS[:2] + ["ngrid", "features"], names)
            psdk.update(pn, tn, mf, tuple(shape))
            assert pn.tensor.shape == pf.shape and pn.names[2] == "ngrid"
            out[f"pred{step}"], out[f"target{step}"], out[f"mask{step}"] = pf.numpy(), tf.numpy(), mf.numpy()
        else:
            psdk.update(NT(p, DIMS, names), NT(t, DIMS, names), mask, None)
            psdvar.update(NT(p, DIMS, names), NT(t, DIMS, names), mask, None)
            out[f"pred{step}"], out[f"target{step}"], out[f"mask{step}"] = p.numpy(), t.numpy(), mask.numpy()
            out[f"sum_rmse{step}"] = psdvar.sum_rmse.clone().numpy()
        out[f"sum_psd_pred{step}"] = psdk.sum_psd_pred.clone().numpy()
        out[f"sum_psd_target{step}"] = psdk.sum_psd_target.clone().numpy()
    out["rmax"] = np.int64(out["psd_pred0"].shape[1])
    del PLOTTED[:]
    res = psdk.compute(prefix="val")
    out["psdk_keys"] = np.array(list(res.keys()))
    out["plot_k"] = PLOTTED[0][0]
    out["plot_pred"] = np.stack([p[1] for p in PLOTTED])
    out["plot_target"] = np.stack([p[2] for p in PLOTTED])
    out["plot_titles"] = np.array([p[3] for p in PLOTTED])
    assert float(psdk.step_count) == 0.0
    if psdvar is not None:
        res = psdvar.compute(prefix="val")
        out["rmse_keys"] = np.array(list(res.keys()))
        out["rmse_vals"] = np.array([float(v) for v in res.values()], dtype=np.float32)
    path = os.path.join(HERE, f"psd_{name}.npz")
    np.savez_compressed(path, **out)
    return path


def gen_rmax(metrics):
    """Rmax (the length of the profile) on the shapes the closed form was checked on"""
    shapes = [(2, 16, 16), (2, 64, 64), (3, 24, 40), (2, 40, 24), (2, 17, 33), (1, 512, 512), (2, 512, 640)]
    g = np.random.default_rng(3)
    rmax = [metrics.power_spectral_density(g.standard_normal((1, 1) + s[1:]).astype(np.float32)).shape[1] for s in shapes]
    np.savez_compressed(os.path.join(HERE, "psd_rmax.npz"), shapes=np.array(shapes, dtype=np.int64), rmax=np.array(rmax, dtype=np.int64))


if __name__ == "__main__":
    m = load_reference()
    gen_case(m, "case0", 101, (3, 3, 24, 40, 5), 2)
    gen_case(m, "case1", 102, (2, 2, 40, 24, 8), 0)
    gen_case(m, "case2", 103, (2, 1, 17, 33, 7), 0)
    gen_case(m, "flat", 104, (2, 2, 12, 18, 3), 1, flat=True)
    gen_rmax(m)
    for f in sorted(f for f in os.listdir(HERE) if f.startswith("psd_") and f.endswith(".npz")):
        print(f, os.path.getsize(os.path.join(HERE, f)))
