"""
Native score-card and spatial-error observers: ``StateErrorPlot`` and ``SpatialErrorPlot`` of ``py4cast/plots.py:488-651`` with the
same interface (``update(obj, batch, prediction, target, mask)``, ``on_step_end(obj, label)``, the constructor arguments) and the
same products -- the ``{label}_{name}/timestep_{feature}`` scalars, ``{label}_{name}_scores.json``, the score cards, the spatial
error maps -- without the ``py4cast`` package, cartopy or tueplots.

Where the reference makes three passes over prediction and target per step (``ScaledLoss`` for mae, for rmse,
``WeightedLoss(reduce_spatial_dim=False)``; a fourth over the target with ``mask_on_nan``), each followed by a collective and a
blocking host copy, the plotters of one step here share ONE ``ops.eval_sums`` call (``p4c_eval_sums``) and keep their state on the
device: a float64 running sum over samples of each score (T,F), the running sum of the error map (T,*S) and the sample count.
``update`` makes no host copy and no collective; ``on_step_end`` makes one sum all-reduce (when ``torch.distributed`` is
initialised) and one copy, and divides by the global sample count -- the reference's mean over ranks followed by the mean over the
concatenated batches, ranks having equal batch shapes there.

The shared pass is taken when ``metrics`` holds only ``ScaledLoss`` members on L1Loss / MSELoss (scores) and ``obj.loss`` is a
single ``WeightedLoss`` on one of them, bare or as the only member (weight 1) of a ``CombinedLoss`` (map); anything else calls the metric objects / ``obj.loss`` as the reference does and feeds
the same state.  Figures are plain matplotlib; without matplotlib they are skipped and everything else is still produced.

``PredictionTimestepPlot`` and ``PredictionEpochPlot`` (``plots.py:242-485``) are here as well, at the end of the module: the
reference's constructor, bookkeeping and output names around ``ops.map_planes`` + ``ops.map_render`` (``csrc/map_frames.hip``),
which make finished RGB frames of the drawn samples and variables on the device; no map projection.
"""

import json
import weakref
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import ops
from .losses import CombinedLoss, ScaledLoss, WeightedLoss, _mask_spec
from .namedtensor import NamedTensor

# ------------------------------------------------------------------------------------------------ the shared pass
_LAST_STEP = [None]   # the last ops.eval_sums call: weak references to prediction / target / mask, their versions, the results


def _ref(obj):
    return None if obj is None else weakref.ref(obj)


def _fusable_metrics(metrics: dict) -> bool:
    return bool(metrics) and all(isinstance(m, ScaledLoss) and m.fused_capable for m in metrics.values())


def _fusable_loss(loss) -> Optional[WeightedLoss]:
    """the single WeightedLoss on L1Loss / MSELoss behind ``obj.loss`` -- itself, or the only member (weight 1) of the CombinedLoss
    the Lightning module wraps its yaml losses in -- or None"""
    if isinstance(loss, CombinedLoss) and len(loss.losses) == 1 and loss.losses[0][1] == 1.0:
        loss = loss.losses[0][0]
    return loss if isinstance(loss, WeightedLoss) and loss.fused_capable else None


def _step_sums(obj, prediction: NamedTensor, target: NamedTensor, mask, scaled: Optional[ScaledLoss] = None, spatial=None,
               collect: bool = False) -> dict:
    """The step's ``ops.eval_sums`` result, computed once for the plotters that are notified with the same objects one after the
    other (lightning._notify).  ``scaled``: a prepared ScaledLoss (std, interior) when scores are wanted.  ``spatial``: the
    SpatialErrorPlot whose running map takes the step's map (``obj.loss`` is then a fusable WeightedLoss) -- passed by that plotter
    itself with ``collect=True``, or by a StateErrorPlot on its behalf; the entry then carries ``map_pending`` until the plotter's
    own ``update`` collects it, so a step's map is added exactly once."""
    spec, tgt = _mask_spec(mask, target)
    objs = (prediction.tensor, tgt, mask)
    versions = tuple(o._version if isinstance(o, torch.Tensor) else None for o in objs)   # (a lazy marker is not asked: it would build)
    try:
        refs = tuple(_ref(o) for o in objs)
    except TypeError:   # a mask object that cannot be weakly referenced: nothing is shared, every plotter makes its own call
        refs = None
        if not collect:
            spatial = None
    last = _LAST_STEP[0]
    if refs is not None and last is not None and last["versions"] == versions and all(
            (r is None and o is None) or (r is not None and r() is o) for r, o in zip(last["refs"], objs)):
        mapped = last["spatial"] is not None and last["spatial"]() is spatial
        if collect and mapped and last["map_pending"]:
            last["map_pending"] = False
            return last
        if not collect and last["has_scores"]:
            return last
        if not collect and mapped:
            spatial = None   # this step's map is already in: only the scores are missing
    loss = _fusable_loss(getattr(obj, "loss", None))
    device, names = prediction.tensor.device, tuple(prediction.feature_names)
    src = scaled if scaled is not None else loss
    std = src.weights(names, device)          # (without metrics the scores are not read)
    interior, num_interior = src._interior_flat(src.lm, device), src.num_interior
    weights, map_kind, map_acc, accumulate = None, None, None, False
    if spatial is not None:
        weights, map_kind = loss.weights(names, device), loss.kind
        shape = (prediction.tensor.shape[1],) + tuple(prediction.tensor.shape[2:-1])
        accumulate = spatial.map_acc is not None
        if not accumulate:
            spatial.map_acc = torch.empty(shape, dtype=torch.float32, device=device)
        map_acc = spatial.map_acc
    scores, count = ops.eval_sums(prediction.tensor, tgt, spec, std, interior, num_interior, weights, map_kind, map_acc, accumulate)
    entry = {"refs": refs, "versions": versions, "scores": scores, "masked_count": count, "has_scores": scaled is not None,
             "spatial": _ref(spatial), "map_pending": spatial is not None and not collect}
    _LAST_STEP[0] = entry if refs is not None else None
    return entry


# ------------------------------------------------------------------------------------------------ state across ranks
def pack_state(tensors: Sequence[torch.Tensor], count) -> torch.Tensor:
    """Running sums and the sample count as one flat float64 tensor: what a rank contributes to the sum all-reduce."""
    device = tensors[0].device
    return torch.cat([t.reshape(-1).double() for t in tensors] + [torch.tensor([float(count)], dtype=torch.float64, device=device)])


def merge_mean(flat_sum: torch.Tensor, shapes: Sequence[Sequence[int]]) -> List[torch.Tensor]:
    """The means over all samples from the SUM of the ranks' ``pack_state`` tensors.  Equal to the reference's mean over ranks
    followed by the mean over the concatenated batches (plots.py:522-526, 541-542) when ranks have equal batch shapes."""
    count = flat_sum[-1]
    out, start = [], 0
    for shape in shapes:
        n = int(np.prod(shape)) if len(shape) else 1
        out.append((flat_sum[start:start + n] / count).reshape(tuple(shape)))
        start += n
    return out


def _reduce_mean(tensors: Sequence[torch.Tensor], count) -> List[torch.Tensor]:
    """one all-reduce (when torch.distributed runs), one device-to-host copy"""
    flat = pack_state(tensors, count)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.all_reduce(flat, op=torch.distributed.ReduceOp.SUM)
    return merge_mean(flat.cpu(), [tuple(t.shape) for t in tensors])


# ------------------------------------------------------------------------------------------------ host side
def _trainer_flag(obj, name: str, default):
    value = getattr(getattr(obj, "trainer", None), name, None)
    return default if value is None else bool(value)


def _is_global_zero(obj) -> bool:
    distributed = torch.distributed.is_available() and torch.distributed.is_initialized()
    return _trainer_flag(obj, "is_global_zero", not distributed or torch.distributed.get_rank() == 0)


def _experiment(obj):
    logger = getattr(obj, "logger", None)
    if logger is None:
        logger = getattr(getattr(obj, "trainer", None), "logger", None)
    return getattr(logger, "experiment", None)


def _pyplot():
    try:
        import matplotlib

        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt

        return plt
    except Exception:   # noqa: BLE001  (matplotlib absent or unusable: no figures)
        return None


def _hand_on(obj, fig, name: str, step: int, dest: Optional[Path], artifact: Optional[str] = None):
    """a figure to the logger's experiment, to a png and to mlflow, as plots.py:561-576 does (``artifact``: the mlflow file name
    where it is not ``name``)"""
    experiment = _experiment(obj)
    if experiment is not None and hasattr(experiment, "add_figure"):
        experiment.add_figure(name, fig, step)
    if dest is not None:
        dest.parent.mkdir(parents=True, exist_ok=True)
        fig.savefig(dest)
    mlflow_logger = getattr(obj, "mlflow_logger", None)
    if mlflow_logger:
        mlflow_logger.experiment.log_figure(run_id=mlflow_logger.version, figure=fig, artifact_file=f"figures/{artifact or name}.png")


def plot_score_card(errors: np.ndarray, shortnames, units, title=None, step_duration=3):
    """Feature x lead-time grid of ``errors`` (T,F) with the values annotated, coloured per feature (each row scaled by its
    maximum), after plots.py:48-93.  None without matplotlib."""
    plt = _pyplot()
    if plt is None:
        return None
    errors_np = np.asarray(errors, dtype=np.float64).T   # (F, T)
    d_f, pred_steps = errors_np.shape
    max_errors = errors_np.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        errors_norm = np.where(max_errors > 0, errors_np / max_errors, 0.0)
    fig, ax = plt.subplots(figsize=(max(4.0, 1.2 * pred_steps + 3.0), max(3.0, 0.45 * d_f + 1.5)))
    ax.imshow(errors_norm, cmap="OrRd", vmin=0, vmax=1.0, interpolation="none", aspect="auto", alpha=0.8)
    for (j, i), error in np.ndenumerate(errors_np):
        ax.text(i, j, f"{error:.3f}" if error < 9999 else f"{error:.2E}", ha="center", va="center")
    ax.set_xticks(np.arange(pred_steps))
    ax.set_xticklabels(step_duration * (np.arange(pred_steps) + 1))
    ax.set_xlabel("Lead time (h)")
    ax.set_yticks(np.arange(d_f))
    ax.set_yticklabels([f"{name} ({unit})" if unit else f"{name}" for name, unit in zip(shortnames, units)], rotation=30)
    if title:
        ax.set_title(title)
    fig.tight_layout()
    plt.close(fig)
    return fig


def plot_spatial_error(error: np.ndarray, interior: Optional[np.ndarray], title=None):
    """``imshow`` of one (H,W) error map, the border region faded through the interior mask (plots.py:167-211 without the map
    projection).  None without matplotlib."""
    plt = _pyplot()
    if plt is None:
        return None
    fig, ax = plt.subplots(figsize=(5, 4.8))
    alpha = None if interior is None else np.clip(np.asarray(interior, dtype=np.float64), 0.7, 1.0)
    im = ax.imshow(np.asarray(error), origin="lower", alpha=alpha, cmap="OrRd")
    cbar = fig.colorbar(im, aspect=30)
    cbar.formatter.set_powerlimits((-3, 3))
    if title:
        fig.suptitle(title, size=10)
    plt.close(fig)
    return fig


# ------------------------------------------------------------------------------------------------ the plotters
class StateErrorPlot:
    """The error of each variable against the lead time (plots.py:488-586): scalars, JSON and a score card per metric.
    ``map_consumer``: a SpatialErrorPlot notified right after this plotter with the same objects (lightning.on_test_start sets
    it); the step's single pass then fills its map too."""

    def __init__(self, metrics: Dict[str, object], prefix: str = "Test", save_path: Path = None):
        self.metrics = metrics
        self.prefix = prefix
        self.save_path = None if save_path is None else Path(save_path)
        self.shortnames, self.units, self.initialized = [], [], False
        self.map_consumer = None
        self.last_means = {}
        self._clear()

    def _clear(self):
        self.sums = {}    # name -> float64 (T,F) sum over samples, on the device
        self.count = 0    # samples

    def update(self, obj, batch, prediction: NamedTensor, target: NamedTensor, mask) -> None:
        if prediction.tensor.is_cuda and _fusable_metrics(self.metrics):
            first = next(iter(self.metrics.values()))
            consumer = self.map_consumer if _fusable_loss(getattr(obj, "loss", None)) is not None else None
            scores = _step_sums(obj, prediction, target, mask, scaled=first, spatial=consumer)["scores"]
            values = {name: scores[0 if m.kind == L.LOSS_L1 else 1] for name, m in self.metrics.items()}
        else:
            values = {name: m(prediction, target, mask) for name, m in self.metrics.items()}
        for name, value in values.items():   # (B,T,F)
            total = value.double().sum(dim=0)
            self.sums[name] = total if name not in self.sums else self.sums[name] + total
        self.count += prediction.tensor.shape[0]
        if not self.initialized:
            self.shortnames = list(prediction.feature_names)
            units = getattr(getattr(obj, "dataset_info", None), "units", None) or {}
            self.units = [units.get(name, "") for name in self.shortnames]
            self.initialized = True

    def on_step_end(self, obj, label: str = "") -> None:
        if not self.count or not self.sums:
            self._clear()
            return
        names = list(self.sums)
        means = dict(zip(names, _reduce_mean([self.sums[n] for n in names], self.count)))   # host, float64 (T,F)
        self.last_means = means
        self._clear()
        if not _is_global_zero(obj):
            return
        experiment = _experiment(obj)
        step_duration = getattr(getattr(obj, "dataset_info", None), "pred_step", 1)
        for name, loss in means.items():
            loss_dict = {shortname: [float(v) for v in loss[:, k]] for k, shortname in enumerate(self.shortnames)}
            if experiment is not None and hasattr(experiment, "add_scalar"):
                for t in range(loss.shape[0]):
                    for k, shortname in enumerate(self.shortnames):
                        experiment.add_scalar(f"{label}_{name}/timestep_{shortname}", float(loss[t, k]), t + 1)
            if _trainer_flag(obj, "sanity_checking", False):
                continue
            fig = plot_score_card(loss.numpy(), self.shortnames, self.units, step_duration=step_duration)
            if fig is not None:
                fig_name = f"score_cards/{self.prefix}_{name}"
                dest = None if self.save_path is None else self.save_path / f"{fig_name}.png"
                _hand_on(obj, fig, fig_name, int(getattr(obj, "current_epoch", 0) or 0), dest)
            if self.save_path is not None:
                self.save_path.mkdir(parents=True, exist_ok=True)
                with open(self.save_path / f"{label}_{name}_scores.json", "w") as json_file:
                    json.dump(loss_dict, json_file)


class SpatialErrorPlot:
    """Where the errors accumulate, all variables together (plots.py:589-651): one map per lead time."""

    def __init__(self, prefix: str = "Test"):
        self.prefix = prefix
        self.last_mean_map = None
        self._clear()

    def _clear(self):
        self.map_acc = None   # fp32 (T,*S) sum over samples, on the device
        self.count = 0

    def update(self, obj, batch, prediction: NamedTensor, target: NamedTensor, mask) -> None:
        loss = getattr(obj, "loss", None)
        if prediction.tensor.is_cuda and _fusable_loss(loss) is not None:
            _step_sums(obj, prediction, target, mask, scaled=None, spatial=self, collect=True)   # adds the step's map to self.map_acc
        else:
            total = loss(prediction, target, mask, reduce_spatial_dim=False).float().sum(dim=0)
            self.map_acc = total if self.map_acc is None else self.map_acc + total
        self.count += prediction.tensor.shape[0]

    def on_step_end(self, obj, label: str = "") -> None:
        if not self.count or self.map_acc is None:
            self._clear()
            return
        (mean_map,) = _reduce_mean([self.map_acc], self.count)   # host, float64 (T,*S)
        self._clear()
        if mean_map.dim() == 2:   # graph layout: plots.py:608-611
            mean_map = mean_map.reshape(mean_map.shape[0], int(obj.grid_shape[0]), -1)
        self.last_mean_map = mean_map
        if not _is_global_zero(obj) or _trainer_flag(obj, "sanity_checking", False):
            return
        interior = getattr(obj, "interior_2d", None)
        interior = None if interior is None else interior[:, :, 0].detach().float().cpu().numpy()
        pred_step = getattr(getattr(obj, "dataset_info", None), "pred_step", 1)
        for t_i, loss_map in enumerate(mean_map):
            fig = plot_spatial_error(loss_map.numpy(), interior, title=f"{self.prefix} loss, t={t_i} ({pred_step * t_i} h)")
            if fig is None:
                break
            _hand_on(obj, fig, f"spatial_error_{label}/{self.prefix}_loss", t_i, None)


# ------------------------------------------------------------------------------------------------ prediction maps
def plasma_table() -> Optional[np.ndarray]:
    """matplotlib's ``plasma`` as the (256,3) uint8 colour table of ``ops.map_render``; None without matplotlib"""
    try:
        import matplotlib

        return np.ascontiguousarray(matplotlib.colormaps["plasma"](np.arange(256), bytes=True)[:, :3], dtype=np.uint8)
    except Exception:   # noqa: BLE001  (matplotlib absent or unusable)
        return None


def plot_prediction_frame(frame: np.ndarray, vmin: float, vmax: float, title=None):
    """One rendered frame (H, 2W+MAP_GAP, 3) as the reference's two-panel figure (plots.py:113-163 without the map projection):
    the halves under "Ground Truth" and "Prediction", one colour bar on the frame's range.  None without matplotlib."""
    plt = _pyplot()
    if plt is None:
        return None
    from matplotlib.cm import ScalarMappable
    from matplotlib.colors import Normalize

    H, W = frame.shape[0], (frame.shape[1] - ops.MAP_GAP) // 2
    fig, axes = plt.subplots(1, 2, figsize=(13, 7))
    extent = (-0.5, W - 0.5, -0.5, H - 0.5)   # the frame's top row is the grid's last: the axes count as origin="lower" does
    for ax, panel, name in zip(axes, (frame[:, :W], frame[:, W + ops.MAP_GAP:]), ("Ground Truth", "Prediction")):
        ax.imshow(panel, extent=extent, interpolation="none")
        ax.set_title(name, size=15)
    if np.isfinite(vmin) and np.isfinite(vmax):
        cbar = fig.colorbar(ScalarMappable(norm=Normalize(vmin=vmin, vmax=vmax), cmap="plasma"), ax=list(axes), aspect=30)
        cbar.ax.tick_params(labelsize=10)
    if title:
        fig.suptitle(title, size=20)
    plt.close(fig)
    return fig


def write_gif(frames: np.ndarray, dest: Path) -> None:
    """(T,H,W,3) uint8 frames -> a looping GIF, 250 ms per frame (plots.py:349-359), written with PIL from the frames themselves"""
    from PIL import Image

    images = [Image.fromarray(np.ascontiguousarray(f), mode="RGB") for f in frames]
    dest.parent.mkdir(parents=True, exist_ok=True)
    images[0].save(dest, format="GIF", append_images=images[1:], save_all=True, duration=250, loop=0)


class MapPlot:
    """What PredictionTimestepPlot and PredictionEpochPlot share (plots.py:242-346): the reference's constructor and bookkeeping --
    rank zero only, ``min(B, remaining)`` samples until ``num_samples_to_plot`` are drawn, the first ``num_features_to_plot``
    variables or all -- around ONE ``ops.map_planes`` call, ONE ``ops.map_render`` call and ONE asynchronous copy of the frames
    and their colour ranges to pinned host memory, where the reference rescales the whole prediction and target and fetches a
    strided plane per (lead time, variable, panel).  ``lut``: a (256,3) uint8 colour table instead of matplotlib's plasma
    (without matplotlib and without a table nothing can be rendered; with one the GIF is still written)."""

    last_step_only = False   # render only the last lead time (the colour range still spans all of them)

    def __init__(self, num_samples_to_plot: int, num_features_to_plot: Optional[int] = None, prefix: str = "Test",
                 save_path: Path = None, lut=None):
        self.num_samples_to_plot = num_samples_to_plot
        self.plotted_examples = 0
        self.prefix = prefix
        self.num_features_to_plot = num_features_to_plot
        self.save_path = None if save_path is None else Path(save_path)
        self._lut_host = None if lut is None else np.ascontiguousarray(np.asarray(lut), dtype=np.uint8).reshape(256, 3)
        self._cache = {}   # device-side constants: colour table, interior mask, std / mean

    # ---- bookkeeping (host only)
    def remaining(self, obj, batch_size: int) -> int:
        """how many leading samples of this batch are drawn (plots.py:284-291)"""
        if not _is_global_zero(obj) or self.plotted_examples >= self.num_samples_to_plot:
            return 0
        return min(int(batch_size), self.num_samples_to_plot - self.plotted_examples)

    def feature_names(self, prediction: NamedTensor) -> List[str]:
        names = list(prediction.feature_names)
        return names[: self.num_features_to_plot] if self.num_features_to_plot else names   # plots.py:315-319

    @staticmethod
    def units(obj, names: Sequence[str]) -> List[str]:
        units = getattr(getattr(obj, "dataset_info", None), "units", None) or {}
        return [units.get(name, "") for name in names]

    @staticmethod
    def pred_step(obj):
        step = getattr(getattr(obj, "dataset_info", None), "pred_step", None)
        return 1 if step is None else step   # without a step duration the lead time counts steps

    @staticmethod
    def grid(obj, prediction: NamedTensor):
        """(H, W) of the maps; the graph layout (B,T,N,F) unfolds through ``obj.grid_shape`` (plots.py:276-282)"""
        shape = tuple(prediction.tensor.shape[2:-1])
        if len(shape) == 1:
            H = int(obj.grid_shape[0])
            return H, shape[0] // H
        return int(shape[0]), int(shape[1])

    def table(self) -> Optional[np.ndarray]:
        if self._lut_host is None:
            self._lut_host = plasma_table()   # taken from matplotlib once
        return self._lut_host

    # ---- device side
    def _constants(self, obj, prediction: NamedTensor, H: int, W: int):
        dev, names = prediction.tensor.device, tuple(prediction.feature_names)
        key = (dev, names, H, W)
        if self._cache.get("key") != key:
            interior = getattr(obj, "interior_2d", None)
            interior = (torch.ones(H * W, dtype=torch.float32, device=dev) if interior is None
                        else interior[:, :, 0].detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous())
            self._cache = {
                "key": key, "interior": interior, "lut": torch.from_numpy(self.table()).to(dev),
                "std": obj.stats.to_list("std", list(names)).to(device=dev, dtype=torch.float32),
                "mean": obj.stats.to_list("mean", list(names)).to(device=dev, dtype=torch.float32),
            }
        return self._cache

    def render(self, obj, prediction: NamedTensor, target: NamedTensor, mask, n: int, K: int):
        """-> (frames (n,T',K,H,2W+G,3) uint8, vrange (n,K,2) float32) as numpy views of one pinned buffer, complete"""
        H, W = self.grid(obj, prediction)
        c = self._constants(obj, prediction, H, W)
        spec, tgt = _mask_spec(mask, target)
        planes, vrange = ops.map_planes(prediction.tensor, tgt, spec, c["std"], c["mean"], range(K), n)
        if self.last_step_only:
            planes = planes[:, -1:].contiguous()
        shape = tuple(planes.shape[:3]) + (H, 2 * W + ops.MAP_GAP, 3)
        nbytes = int(np.prod(shape))
        tail = (nbytes + 3) // 4 * 4
        packed = torch.empty(tail + 4 * vrange.numel(), dtype=torch.uint8, device=planes.device)   # frames, then the ranges
        ops.map_render(planes, vrange, c["lut"], c["interior"], H, W, out=packed[:nbytes].view(shape))
        packed[tail:].view(torch.float32).copy_(vrange.reshape(-1))
        host = torch.empty(packed.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(packed, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(planes.device))
        done.synchronize()   # the figures are composed at once, as the reference does inside update
        flat = host.numpy()
        return flat[:nbytes].reshape(shape), flat[tail:].view(np.float32).reshape(tuple(vrange.shape))

    def update(self, obj, batch, prediction: NamedTensor, target: NamedTensor, mask) -> None:
        n = self.remaining(obj, prediction.tensor.shape[0])
        if n == 0:
            return
        names = self.feature_names(prediction)
        if self.table() is None:   # no matplotlib and no table: nothing to draw with
            self.plotted_examples += n
            return
        frames, vrange = self.render(obj, prediction, target, mask, n, len(names))
        for s in range(n):
            self.plotted_examples += 1   # plots.py:309
            self.plot_map(obj, frames[s], vrange[s], names)

    def plot_map(self, obj, frames: np.ndarray, vrange: np.ndarray, names: List[str]) -> None:  # pragma: no cover - abstract
        raise NotImplementedError

    def on_step_end(self, obj, label: str = "") -> None:
        pass


class PredictionTimestepPlot(MapPlot):
    """Prediction against target for each lead time, and a GIF per variable (plots.py:362-423)."""

    def titles(self, obj, names: Sequence[str], t_i: int) -> List[str]:
        step = self.pred_step(obj)
        return [f"{name} ({unit}), t={t_i} ({step * t_i} h)" for name, unit in zip(names, self.units(obj, names))]

    def plot_map(self, obj, frames, vrange, names) -> None:
        for t_i in range(1, frames.shape[0] + 1):
            for k, (name, title) in enumerate(zip(names, self.titles(obj, names, t_i))):
                fig = plot_prediction_frame(frames[t_i - 1, k], float(vrange[k, 0]), float(vrange[k, 1]), title=title)
                if fig is None:
                    break
                fig_name = f"timestep_evol_per_param/{name}_example_{self.plotted_examples}"
                dest = None if self.save_path is None else self.save_path / f"{fig_name}_{t_i}.png"
                _hand_on(obj, fig, fig_name, t_i, dest, artifact=f"{fig_name}_{t_i}")
        if self.save_path is not None and frames.shape[0] > 1:   # plots.py:419-423
            for k, name in enumerate(names):
                write_gif(frames[:, k], self.save_path / f"timestep_evol_per_param/{name}.gif")


class PredictionEpochPlot(MapPlot):
    """Prediction against target at the last lead time, once per epoch (plots.py:426-485)."""

    last_step_only = True

    def titles(self, obj, names: Sequence[str], max_step: int) -> List[str]:
        leadtime, epoch = self.pred_step(obj) * max_step, int(getattr(obj, "current_epoch", 0) or 0)
        return [f"{name} ({unit}), t={max_step} ({leadtime} h) - epoch {epoch}" for name, unit in zip(names, self.units(obj, names))]

    def render(self, obj, prediction, target, mask, n, K):
        self._max_step = int(prediction.tensor.shape[1])
        return super().render(obj, prediction, target, mask, n, K)

    def plot_map(self, obj, frames, vrange, names) -> None:
        epoch = int(getattr(obj, "current_epoch", 0) or 0)
        for k, (name, title) in enumerate(zip(names, self.titles(obj, names, self._max_step))):
            fig = plot_prediction_frame(frames[-1, k], float(vrange[k, 0]), float(vrange[k, 1]), title=title)
            if fig is None:
                break
            fig_name = f"epoch_evol_per_param/{name}_example_{self.plotted_examples}"
            dest = None if self.save_path is None else self.save_path / f"{fig_name}_{epoch}.png"
            _hand_on(obj, fig, fig_name, epoch, dest, artifact=f"{fig_name}_{epoch}")
