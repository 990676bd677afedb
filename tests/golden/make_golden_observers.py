#!/usr/bin/env python3
"""
Golden vectors for the score-card and spatial-error observers -- runs ONLY in the build container (needs the reference).

Executes the reference's unmodified ``StateErrorPlot`` and ``SpatialErrorPlot`` (``py4cast/plots.py:488-651``) with its unmodified
``ScaledLoss`` and ``WeightedLoss`` (``py4cast/losses.py:103-210``) on the CPU, through the ``sys.modules`` stubs of
``make_golden.py`` plus stubs for what ``plots.py`` imports and this machine lacks (cartopy, tueplots, torchmetrics, gif).  The two
figure functions ``plot_error_map`` and ``plot_spatial_error`` are replaced by stubs that draw nothing and record their arguments;
the trainer's strategy reduces by identity (one rank) and the logger's ``experiment`` records ``add_scalar`` / ``add_figure``.

Each case makes two ``update`` calls, then ``on_step_end``, all in grid form (B,T,H,W,F).  Stored per case: the inputs, the
per-update (B,T,F) scores and (B,T,H,W) maps the plotters appended, the final (T,F) means and (T,H,W) mean map handed to the figure
functions, the scalar names / steps / values and the JSON files as written.

    python tests/golden/make_golden_observers.py
"""

import importlib
import json
import os
import shutil
import sys
import tempfile
import types
from pathlib import Path

import matplotlib

matplotlib.use("Agg")
import matplotlib.figure  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (stub helpers, NamedTensor shim)

DIMS = ["batch", "timestep", "lat", "lon", "features"]
RECORDED = {"error_map": [], "spatial": []}


class FakeFigure(matplotlib.figure.Figure):   # (plt.close insists on a Figure; nothing is drawn on it)
    def savefig(self, dest, *a, **k):
        Path(dest).write_bytes(b"")


def plot_error_map(errors, shortnames, units, title=None, step_duration=3):
    RECORDED["error_map"].append((errors.clone().numpy(), list(shortnames), list(units), step_duration))
    return FakeFigure()


def plot_spatial_error(error, obs_mask, domain_info, title=None, vrange=None):
    RECORDED["spatial"].append((error.clone().numpy(), obs_mask.clone().numpy(), title))
    return FakeFigure()


def load_reference():
    losses, _ = mg.install_stubs()
    del sys.modules["py4cast.plots"]   # make_golden's placeholder: the real file is imported below
    crs = types.ModuleType("cartopy.crs")
    mg.stub("cartopy", crs=crs)
    sys.modules["cartopy.crs"] = crs
    bundle = lambda **k: {"figure.figsize": (6.0, 4.0)}  # noqa: E731
    mg.stub("tueplots", bundles=types.SimpleNamespace(neurips2023=bundle), figsizes=types.SimpleNamespace(neurips2023=lambda **k: {}))
    mg.stub("torchmetrics", Metric=torch.nn.Module)
    try:
        import PIL  # noqa: F401
    except ImportError:
        mg.stub("PIL", Image=None)
    plots = importlib.import_module("py4cast.plots")  # unmodified reference file
    plots.plot_error_map, plots.plot_spatial_error = plot_error_map, plot_spatial_error
    return losses, plots


class Experiment:
    def __init__(self):
        self.scalars, self.figures = [], []

    def add_scalar(self, name, value, step):
        self.scalars.append((name, float(value), int(step)))

    def add_figure(self, name, fig, step):
        self.figures.append((name, int(step)))


def gen_case(losses, plots, name, seed, shape, border, mask_kind, map_loss):
    g = torch.Generator().manual_seed(seed)
    B, T, H, W, F = shape
    names = [f"f{i}" for i in range(F)]
    std, diff_std, state_weight = torch.rand(F, generator=g) + 0.5, torch.rand(F, generator=g) + 0.5, 1.0 + torch.rand(F, generator=g)
    bm = torch.zeros(H, W, 1)
    bm[:border], bm[-border:], bm[:, :border], bm[:, -border:] = 1, 1, 1, 1
    interior = 1.0 - bm

    lm = torch.nn.Module()

    class DI:
        state_weights = {n: float(state_weight[i]) for i, n in enumerate(names)}
        stats = mg.StatsLike({n: {"std": std[i]} for i, n in enumerate(names)})
        diff_stats = mg.StatsLike({n: {"std": diff_std[i]} for i, n in enumerate(names)})
        units = {n: f"u{i}" for i, n in enumerate(names)}
        pred_step = 1
        domain_info = None

    metrics = {}
    for torch_loss, alias in ("L1Loss", "mae"), ("MSELoss", "rmse"):
        metrics[alias] = losses.ScaledLoss(torch_loss, reduction="none")
        metrics[alias].prepare(lm, interior, DI)
    loss = losses.WeightedLoss(map_loss, reduction="none")
    loss.prepare(lm, interior, DI)

    exp = Experiment()
    tmp = Path(tempfile.mkdtemp())
    obj = types.SimpleNamespace(
        loss=loss, dataset_info=DI, logger=types.SimpleNamespace(experiment=exp), mlflow_logger=None, current_epoch=0,
        interior_2d=interior, grid_shape=(H, W),
        trainer=types.SimpleNamespace(strategy=types.SimpleNamespace(reduce=lambda t, reduce_op: t), is_global_zero=True,
                                      sanity_checking=False))
    state, spatial = plots.StateErrorPlot(metrics, prefix="Test", save_path=tmp), plots.SpatialErrorPlot(prefix="Test")
    out = {"names": np.array(names), "std": std.numpy(), "diff_std": diff_std.numpy(), "state_weight": state_weight.numpy(),
           "interior": interior.numpy(), "map_loss": np.array(map_loss), "units": np.array([DI.units[n] for n in names])}
    for u in range(2):
        p, t = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        if mask_kind == "none":
            mask, tm = torch.ones_like(t), t                        # lightning.py:797
        elif mask_kind == "float":
            mask, tm = (torch.rand(shape, generator=g) > 0.15).float(), t
        else:                                                       # lightning.py:792-796
            t[torch.rand(shape, generator=g) < 0.05] = float("nan")
            t[:, :, border + 1, border + 2, :] = float("nan")       # NaN for every (b,t,f): one interior point ...
            t[:, :, 0, 1, :] = float("nan")                         # ... and one border point
            if u == 1:
                t[:, :, H - border - 2, border, :] = float("nan")
            mask, tm = ~torch.isnan(t), torch.nan_to_num(t, nan=0)
        pn, tn = mg.NamedTensor(p, DIMS, names), mg.NamedTensor(tm, DIMS, names)
        state.update(obj, None, pn, tn, mask)
        spatial.update(obj, None, pn, tn, mask)
        out[f"pred{u}"], out[f"target{u}"] = p.numpy(), t.numpy()   # the raw target (NaNs in place)
        out[f"mask{u}"] = mask.numpy()
        out[f"mae{u}"], out[f"rmse{u}"] = state.losses["mae"][-1].numpy(), state.losses["rmse"][-1].numpy()
        out[f"map{u}"] = spatial.spatial_loss_maps[-1].numpy()
    RECORDED["error_map"].clear(), RECORDED["spatial"].clear()
    state.on_step_end(obj, label="Test")
    spatial.on_step_end(obj, label="Test")
    assert [r[1] for r in RECORDED["error_map"]] == [names, names]
    out["mean_mae"], out["mean_rmse"] = RECORDED["error_map"][0][0], RECORDED["error_map"][1][0]
    out["mean_map"] = np.stack([r[0] for r in RECORDED["spatial"]])
    out["spatial_titles"] = np.array([r[2] for r in RECORDED["spatial"]])
    out["scalar_names"] = np.array([s[0] for s in exp.scalars])
    out["scalar_values"] = np.array([s[1] for s in exp.scalars], dtype=np.float64)
    out["scalar_steps"] = np.array([s[2] for s in exp.scalars], dtype=np.int64)
    out["figure_names"] = np.array([f[0] for f in exp.figures])
    out["figure_steps"] = np.array([f[1] for f in exp.figures], dtype=np.int64)
    for alias in ("mae", "rmse"):
        out[f"json_{alias}"] = np.array((tmp / f"Test_{alias}_scores.json").read_text())
        assert list(json.loads(str(out[f"json_{alias}"]))) == names
    assert not state.losses["mae"] and not spatial.spatial_loss_maps
    shutil.rmtree(tmp)
    path = os.path.join(HERE, f"observers_{name}.npz")
    np.savez_compressed(path, **out)
    return path


if __name__ == "__main__":
    ref_losses, ref_plots = load_reference()
    gen_case(ref_losses, ref_plots, "case0", 201, (2, 3, 8, 12, 5), 1, "none", "MSELoss")
    gen_case(ref_losses, ref_plots, "case1", 202, (2, 2, 12, 20, 3), 2, "float", "L1Loss")
    gen_case(ref_losses, ref_plots, "case2", 203, (3, 2, 9, 7, 4), 2, "nan", "MSELoss")
    for f in sorted(f for f in os.listdir(HERE) if f.startswith("observers_") and f.endswith(".npz")):
        print(f, os.path.getsize(os.path.join(HERE, f)))
