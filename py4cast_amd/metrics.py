"""
Validation metric next to the losses: the anomaly correlation coefficient of
``py4cast/metrics.py:355-455`` with the spatial reductions done by one HIP kernel (``p4c_acc_sums``) over
prediction and target, instead of five full-tensor torch passes.  Same ``update`` / ``compute`` / ``reset``
contract as the reference's torchmetrics ``Metric`` (state ``sum_acc`` (T,F) and ``step_count``, both summed
across ranks by the caller as ``dist_reduce_fx="sum"`` prescribes).

``MetricPSDK`` and ``MetricPSDVar`` (``py4cast/metrics.py:13-249``) stand on ``ops.psd``: one streaming HIP pass over prediction
and target at the chosen time step instead of a host copy and two ``scipy`` DCTs per feature and sample.  The spectrum is the
reference's as it stands ("Power spectrum"): its radial binning reads row 0 and one corner of the 2-D DCT only.
"""

import warnings
import weakref
from pathlib import Path

import numpy as np
import torch

from . import ops
from .namedtensor import NamedTensor


class MetricACC:
    def __init__(self, dataset_info, device=None):
        warnings.warn(
            "ACC supposes access to climate normals; they are one scalar per field here (metrics.py:362-369)."
        )
        names = dataset_info.shortnames["input_output"] + dataset_info.shortnames["output"]
        self.climate_means = dataset_info.stats.to_list("mean", names)
        if device is not None:
            self.climate_means = self.climate_means.to(device)
        self.reset()

    def reset(self):
        self.sum_acc = torch.tensor(0.0)
        self.step_count = 0.0
        self.feature_names, self.pred_steps = None, None

    def update(self, preds: NamedTensor, target: NamedTensor, mask: torch.Tensor, *args):
        """(B,T,*S,F) prediction / target and a 0/1 mask of the same shape (metrics.py:387-433)."""
        if preds.tensor.shape != target.tensor.shape:
            raise ValueError("preds and target must have the same shape")
        if self.step_count == 0:
            self.climate_means = self.climate_means.to(preds.tensor.device)
            self.feature_names = preds.feature_names
            self.pred_steps = preds.tensor.shape[1]
        from .losses import _mask_spec   # the lazy markers of get_mask_on_nan are read in place (no mask / clean target built)

        spec, tgt = _mask_spec(mask, target)
        sums = ops.acc_sums(preds.tensor, tgt, spec, self.climate_means)
        res = torch.mean(sums[0] / torch.sqrt(sums[1] * sums[2]), dim=0)  # tiny (B,T,F) tail, metrics.py:425
        if not self.sum_acc.ndim:
            self.sum_acc = torch.zeros(self.pred_steps, preds.tensor.shape[-1], device=preds.tensor.device)
        self.sum_acc += res
        self.step_count += 1

    def compute(self, prefix: str = "val") -> dict:
        mean_acc = self.sum_acc / self.step_count
        out = {
            f"{prefix}_acc/{name}_step{j}": mean_acc[j, i]
            for i, name in enumerate(self.feature_names)
            for j in range(self.pred_steps)
        }
        self.reset()
        return out


# ------------------------------------------------------------------------------------------------ power spectrum
_LAST_PSD = [None]   # (weak references to prediction / target / mask, their versions, pred_step, grid, spectra)


def _ref(obj):
    return None if obj is None else weakref.ref(obj)


def _spectra(preds: NamedTensor, targets: NamedTensor, mask, shape, pred_step: int) -> torch.Tensor:
    """(2, F, Rmax) spectra of one ``update``.  The two PSD metrics are notified with the same objects one after the other
    (lightning._notify): the second one takes the first one's result."""
    if preds.tensor.shape != targets.tensor.shape:
        raise ValueError("preds and targets must have the same shape")
    grid = None if shape is None else tuple(int(v) for v in shape[2:4])
    if preds.tensor.dim() != (5 if grid is None else 4):
        raise ValueError("PSD metrics take (B,T,H,W,F) tensors, or (B,T,N,F) tensors with the original shape")
    if grid is not None and grid[0] * grid[1] != preds.tensor.shape[2]:
        raise ValueError(f"shape {tuple(shape)} does not unflatten {preds.tensor.shape[2]} grid points")
    from .losses import _mask_spec   # the lazy markers of get_mask_on_nan are read in place (no mask / clean target built)

    spec, tgt = _mask_spec(mask, targets)
    objs = (preds.tensor, tgt, mask)
    versions = tuple(o._version if isinstance(o, torch.Tensor) else None for o in objs)   # (a lazy marker is not asked: it would build)
    last = _LAST_PSD[0]
    if last is not None and last[1:4] == (versions, pred_step, grid) and all(
            (r is None and o is None) or (r is not None and r() is o) for r, o in zip(last[0], objs)):
        return last[4]
    out = ops.psd(preds.tensor, tgt, spec, pred_step, grid)
    try:
        _LAST_PSD[0] = (tuple(_ref(o) for o in objs), versions, pred_step, grid, out)
    except TypeError:   # a mask object that cannot be weakly referenced: nothing is shared
        _LAST_PSD[0] = None
    return out


def _plot_log_psd(k, psd_pred, psd_target, title: str):
    """log-log figure of the two spectra against the wave number, or None without matplotlib"""
    try:
        import matplotlib

        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
    except Exception:   # noqa: BLE001  (matplotlib absent or unusable: the metric returns no figures)
        return None
    fig, ax = plt.subplots(figsize=(6, 4))
    ax.loglog(k, psd_pred, label="prediction")
    ax.loglog(k, psd_target, label="target")
    ax.set_xlabel("wave number k")
    ax.set_ylabel("power spectral density")
    ax.set_title(title)
    ax.legend()
    fig.tight_layout()
    plt.close(fig)
    return fig


class MetricPSDK:
    """Mean power spectral density against the wave number, per feature, at time step ``pred_step`` (metrics.py:13-144).
    State ``sum_psd_pred`` / ``sum_psd_target`` (F, Rmax) and ``step_count``, summed across ranks by the caller.  With ``shape``
    the flattened (B,T,N,F) tensors are read as ``shape[2:4]`` grids; the caller's tensors stay flattened."""

    def __init__(self, save_path, pred_step: int = 0):
        self.save_path = None if save_path is None else Path(save_path)
        self.pred_step = pred_step
        self.last_mean_psd_pred, self.last_mean_psd_target = None, None
        self.reset()

    def reset(self):
        self.sum_psd_pred = torch.tensor(0.0)
        self.sum_psd_target = torch.tensor(0.0)
        self.step_count = 0.0
        self.feature_names = None

    def update(self, preds: NamedTensor, targets: NamedTensor, mask, shape=None):
        spectra = _spectra(preds, targets, mask, shape, self.pred_step)
        if self.step_count == 0:
            self.feature_names = preds.feature_names
            self.sum_psd_pred, self.sum_psd_target = torch.zeros_like(spectra[0]), torch.zeros_like(spectra[1])
        self.sum_psd_pred += spectra[0]
        self.sum_psd_target += spectra[1]
        self.step_count += 1

    def compute(self, prefix: str = "val") -> dict:
        """One figure per feature under ``{prefix}_mean_psd_k/{name}`` (none without matplotlib), saved below ``save_path`` when
        it exists; the means stay readable in ``last_mean_psd_pred`` / ``last_mean_psd_target``."""
        if self.step_count == 0:
            return {}
        mean_pred, mean_target = self.sum_psd_pred / self.step_count, self.sum_psd_target / self.step_count
        self.last_mean_psd_pred, self.last_mean_psd_target = mean_pred, mean_target
        rmax = mean_pred.shape[1]
        k = np.linspace(2 * np.pi / 2.6, rmax * 2 * np.pi / 2.6, rmax)   # metrics.py:96
        pred_np, target_np = mean_pred.cpu().numpy(), mean_target.cpu().numpy()
        out = {}
        for c, name in enumerate(self.feature_names):
            fig = _plot_log_psd(k, pred_np[c], target_np[c], f"PSD for {name} at +{self.pred_step + 1}h")
            if fig is None:
                break
            out[f"{prefix}_mean_psd_k/{name}"] = fig
            if self.save_path is not None and self.save_path.exists():
                dest = self.save_path / f"{prefix}_mean_psd_k/{name}_{self.pred_step + 1}.png"
                dest.parent.mkdir(exist_ok=True)
                fig.savefig(dest)
        self.reset()
        return out


class MetricPSDVar:
    """RMSE between the log10 spectra of target and prediction, per feature, at time step ``pred_step`` (metrics.py:147-249).
    State ``sum_rmse`` (F,) and ``step_count``, summed across ranks by the caller.  With ``shape`` the reference forgets to
    unflatten the mask and would raise; here the flattened tensors and mask are read as ``shape[2:4]`` grids."""

    def __init__(self, pred_step: int = 0):
        self.pred_step = pred_step
        self.reset()

    def reset(self):
        self.sum_rmse = torch.tensor(0.0)
        self.step_count = 0.0
        self.feature_names = None

    def update(self, preds: NamedTensor, targets: NamedTensor, mask, shape=None):
        spectra = _spectra(preds, targets, mask, shape, self.pred_step).double()
        res = torch.sqrt(torch.mean((torch.log10(spectra[1]) - torch.log10(spectra[0])) ** 2, dim=1))   # metrics.py:213
        if self.step_count == 0:
            self.feature_names = preds.feature_names
            self.sum_rmse = torch.zeros(res.shape[0], device=res.device)
        self.sum_rmse += res.float()
        self.step_count += 1

    def compute(self, prefix: str = "val") -> dict:
        if self.step_count == 0:
            return {}
        mean = self.sum_rmse / self.step_count
        out = {f"{prefix}_rmse_psd/{name}": mean[i] for i, name in enumerate(self.feature_names)}
        self.reset()
        return out
