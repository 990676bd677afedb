"""
Output staging for the inference path: what happens between the rollout and the GRIB / GIF writers.

The reference (py4cast/lightning.py:1162-1188, py4cast/io/outputs.py:116-241) un-normalises the prediction feature by feature
on the device, then the writers pull ONE (lat, lon) plane per time step and feature with ``tensor[:, :, idx].cpu().numpy()``: a
strided gather plus a synchronous device-to-host copy per plane (3 steps x 60 features = 180 blocking copies per sample).

Here the un-normalisation kernel writes feature-major planes (``p4c_unnormalize_planes``: (B,T,*S,F) -> (B,T,F,*S), bit-exact
with the reference's two rounded steps) and the planes travel to PINNED host buffers with ONE asynchronous copy per batch on a
copy stream.  Two buffers rotate, so the next batch's rollout, the copy of this batch and the host-side writers (CPU-bound:
epygram / matplotlib) of the previous one overlap.  The GRIB writer is the reference's host code (epygram and a template file) and
stays out of scope; it would receive numpy views of the pinned planes -- no further copies.

The GIF writer is native (``ForecastGifWriter``): ``ops.forecast_frames`` turns the normalised prediction into palette-index
frames on the device -- one byte per pixel, every feature of every lead time of the accepted samples, the reference's colour table
and range per parameter (``display_for``) -- the frames and their ranges leave with one asynchronous copy, and the host only wraps
them into "P"-mode GIF frames; no figure is drawn.  ``OutputSavingSettings`` reads the reference's io_conf JSON files.
"""

import json
from dataclasses import dataclass, fields
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .namedtensor import NamedTensor


@dataclass
class StagedPrediction:
    """A batch of un-normalised predictions on the host: ``planes[b, t, f]`` is the contiguous (*spatial) field the writers take."""

    planes: np.ndarray            # (B, T, F, *spatial) float32 view of a pinned buffer -- valid until the slot is reused
    feature_names: List[str]
    names: List[str]              # dimension names of the un-staged tensor (batch, timestep, *spatial, features)
    slot: int

    def plane(self, b: int, t: int, feature: str) -> np.ndarray:
        return self.planes[b, t, self.feature_names.index(feature)]


class OutputStager:
    """``submit`` enqueues kernel + copy and returns at once; ``wait`` blocks on that batch's copy only."""

    def __init__(self, device: torch.device, slots: int = 2):
        if device.type != "cuda":
            raise RuntimeError("OutputStager stages device predictions: it needs the GPU (no CPU fallback)")
        self.device, self.slots = device, slots
        self.copy_stream = torch.cuda.Stream(device=device)
        self._host: List[Optional[torch.Tensor]] = [None] * slots
        self._dev: List[Optional[torch.Tensor]] = [None] * slots
        self._done: List[Optional[torch.cuda.Event]] = [None] * slots
        self._meta = [None] * slots
        self._next = 0

    def _buffers(self, slot: int, shape):
        n = int(np.prod(shape))
        if self._host[slot] is None or self._host[slot].numel() < n:
            self._host[slot] = torch.empty(n, dtype=torch.float32, pin_memory=True)
            self._dev[slot] = torch.empty(n, dtype=torch.float32, device=self.device)
        return self._host[slot][:n].view(shape), self._dev[slot][:n].view(shape)

    def submit(self, preds: NamedTensor, std: torch.Tensor, mean: torch.Tensor) -> int:
        """preds: normalised (B,T,*S,F) on the device.  Returns the slot to pass to ``wait``."""
        slot = self._next
        self._next = (self._next + 1) % self.slots
        if self._done[slot] is not None:
            self._done[slot].synchronize()   # the slot's previous batch must have left the device before its buffers are reused
        t = preds.tensor
        shape = (t.shape[0], t.shape[1], t.shape[-1]) + tuple(t.shape[2:-1])
        host, dev = self._buffers(slot, shape)
        ops.unnormalize_planes(t, std, mean, out=dev)                 # compute stream
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(ready)
            host.copy_(dev, non_blocking=True)                        # one DMA for the whole batch, pinned destination
            done = torch.cuda.Event()
            done.record(self.copy_stream)
        self._done[slot] = done
        self._meta[slot] = (host, list(preds.feature_names), list(preds.names))
        return slot

    def wait(self, slot: int) -> StagedPrediction:
        self._done[slot].synchronize()
        host, feature_names, names = self._meta[slot]
        return StagedPrediction(host.numpy(), feature_names, names, slot)

    def run(self, batches, predict: Callable, std: torch.Tensor, mean: torch.Tensor, write: Callable[[StagedPrediction, int], None]):
        """The inference loop with the overlap spelled out: batch i's writers run while batch i+1 is on the device."""
        pending = None
        for i, batch in enumerate(batches):
            slot = self.submit(predict(batch, i), std, mean)
            if pending is not None:
                write(self.wait(pending[0]), pending[1])
            pending = (slot, i)
        if pending is not None:
            write(self.wait(pending[0]), pending[1])


# ------------------------------------------------------------------------------------------------ forecast GIFs
@dataclass
class OutputSavingSettings:
    """The reference's output settings file (config/IO/*.json; io/outputs.py:17-113): where GRIBs and GIFs go and how they are named.
    ``path_to_runtime`` holds one ``{}`` per entry of ``output_kwargs`` plus a last one for the runtime; ``gif_fmt`` / ``grib_fmt`` one
    per identifier."""

    template_grib: str
    dir_grib: str
    dir_gif: str
    path_to_runtime: str
    grib_fmt: str = "grid.forecast_ai_date_{}_ech_{}.json"
    output_kwargs: Tuple[str, ...] = ()
    grib_identifiers: Tuple[str, ...] = ("date", "leadtime")
    gif_fmt: str = "{}_feature_{}.gif"
    gif_identifiers: Tuple[str, ...] = ("runtime", "feature")

    @classmethod
    def from_json(cls, path) -> "OutputSavingSettings":
        with open(path, "r") as f:
            raw = json.load(f)
        known = {f.name for f in fields(cls)}
        unknown = sorted(set(raw) - known)
        if unknown:
            raise TypeError(f"{path}: unknown output setting(s) {unknown}")
        return cls(**raw)

    def _path(self, root: Path, runtime: str, fmt: str, identifiers: Sequence[str], values: Dict[str, str]) -> Path:
        holes, wanted = fmt.count("{}"), len(identifiers)
        if holes != wanted:
            raise ValueError(f"fmt : {fmt} has {holes} placeholders, but {wanted} identifiers.")
        holes, wanted = self.path_to_runtime.count("{}") - 1, len(self.output_kwargs)   # the last one is the runtime's
        if holes != wanted:
            raise ValueError(f"fmt : {self.path_to_runtime} has {holes} placeholders, but {wanted} identifiers.")
        path = root / self.path_to_runtime.format(*self.output_kwargs, runtime) / fmt.format(*(values[i] for i in identifiers))
        path.parent.mkdir(parents=True, exist_ok=True)
        return path

    def get_gif_path(self, runtime: str, feature: str) -> Path:
        return self._path(Path(self.dir_gif), runtime, self.gif_fmt, self.gif_identifiers, {"runtime": runtime, "feature": feature})


@dataclass(frozen=True)
class FeatureDisplay:
    """How one feature is drawn: the matplotlib colormap, the colour range (None: auto-scaled per frame), the value below which a
    pixel is left blank (None: none) and what is added to the un-normalised value first."""

    cmap: str
    vmin: Optional[float] = None
    vmax: Optional[float] = None
    floor: Optional[float] = None
    offset: float = 0.0


# per parameter -- the second "_" token of a feature name -- as the reference's GIFs show it (utils.py: PARAMS_INFO, plot_frame)
DISPLAY_TABLE = {
    "t2m": FeatureDisplay("Spectral_r", 0.0, 40.0),
    "r2": FeatureDisplay("Spectral", 0.0, 100.0),
    "tp": FeatureDisplay("Spectral_r", 0.5, 60.0, floor=0.5),     # precipitation below 0.5 mm is not drawn
    "u10": FeatureDisplay("RdBu", -20.0, 20.0),
    "v10": FeatureDisplay("RdBu", -20.0, 20.0),
}
DEFAULT_DISPLAY = FeatureDisplay("plasma")
DISPLAY_OFFSETS = {"aro_t2m_2m": -273.15}                          # shown in degrees Celsius (utils.py: make_gif)


def display_for(feature_names: Sequence[str], table: Optional[Dict[str, FeatureDisplay]] = None,
                offsets: Optional[Dict[str, float]] = None) -> List[FeatureDisplay]:
    """One FeatureDisplay per feature name.  ``table``: parameter -> FeatureDisplay (default DISPLAY_TABLE); a parameter it lacks,
    or a name without a second token, is drawn in plasma and auto-scaled.  ``offsets``: full feature name -> offset."""
    table = DISPLAY_TABLE if table is None else table
    offsets = DISPLAY_OFFSETS if offsets is None else offsets
    rows = []
    for name in feature_names:
        tokens = name.split("_")
        row = table.get(tokens[1], DEFAULT_DISPLAY) if len(tokens) > 1 else DEFAULT_DISPLAY
        if name in offsets:
            row = FeatureDisplay(row.cmap, row.vmin, row.vmax, row.floor, float(offsets[name]))
        rows.append(row)
    return rows


def palette_for(cmap: str) -> np.ndarray:
    """(256,3) uint8: entries 0..254 the colormap resampled to 255 colours, entry 255 -- ops.FORECAST_BAD, where matplotlib's
    transparent "bad" colour shows the figure's background -- white"""
    from matplotlib import colormaps

    pal = np.full((256, 3), 255, dtype=np.uint8)
    pal[:255] = colormaps[cmap].resampled(255)(np.arange(255), bytes=True)[:, :3]
    return pal


def save_palette_gif(path, frames: np.ndarray, palette: np.ndarray, duration: int = 500) -> None:
    """frames (T,H,W) uint8 palette indices -> a looping GIF of "P"-mode frames, ``duration`` ms each"""
    from PIL import Image

    images = []
    for frame in frames:
        im = Image.fromarray(np.ascontiguousarray(frame), mode="P")
        im.putpalette(np.ascontiguousarray(palette, dtype=np.uint8).tobytes())
        images.append(im)
    images[0].save(str(path), save_all=True, append_images=images[1:], duration=duration, loop=0, optimize=False)


class ForecastGifWriter:
    """One looping GIF and one ``<gif>.json`` sidecar per (accepted sample, feature) of a predicted batch.

    ``submit`` enqueues ``ops.forecast_frames`` on the current stream and ONE asynchronous copy of frames + ranges into a pinned
    buffer on the copy stream, then encodes what an earlier ``submit`` left pending: batch i's GIFs are written by the host while
    batch i+1 is on the device (the rotation of ``OutputStager.run``).  ``finish(slot)`` waits for that batch's copy only and
    writes its files; ``drain`` finishes what is pending.  ``slots`` pinned / device buffer pairs rotate."""

    def __init__(self, settings: OutputSavingSettings, device: torch.device, slots: int = 2,
                 table: Optional[Dict[str, FeatureDisplay]] = None, offsets: Optional[Dict[str, float]] = None):
        for package, name in (("PIL", "PIL (Pillow)"), ("matplotlib", "matplotlib")):
            try:
                __import__(package)
            except ImportError as exc:
                raise RuntimeError(f"ForecastGifWriter needs {name}: GIF frames are PIL images, colour tables are matplotlib's") from exc
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ForecastGifWriter renders frames on the device: it needs the GPU (no CPU fallback)")
        self.settings, self.device, self.slots = settings, device, slots
        self.table, self.offsets = table, offsets
        self.copy_stream = torch.cuda.Stream(device=device)
        self._host: List[Optional[torch.Tensor]] = [None] * slots
        self._dev: List[Optional[torch.Tensor]] = [None] * slots
        self._done: List[Optional[torch.cuda.Event]] = [None] * slots
        self._meta = [None] * slots
        self._pending: List[int] = []
        self._next = 0
        self._palettes: Dict[str, np.ndarray] = {}
        self.written: List[Path] = []          # every GIF written so far, in order

    def _buffers(self, slot: int, nbytes: int):
        if self._host[slot] is None or self._host[slot].numel() < nbytes:
            self._host[slot] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            self._dev[slot] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._host[slot][:nbytes], self._dev[slot][:nbytes]

    def submit(self, preds: NamedTensor, std: torch.Tensor, mean: torch.Tensor, runtimes: Sequence[str],
               accepted: Sequence[bool]) -> Optional[int]:
        """preds: the NORMALISED prediction (B,T,H,W,F) on the device; ``runtimes[b]`` names sample b's files, ``accepted[b]`` says
        whether it is written.  Returns the slot for ``finish``, or None when no sample is accepted (nothing is launched)."""
        samples = [b for b, ok in enumerate(accepted) if ok]
        earlier = list(self._pending)
        slot = None
        if samples:
            slot = self._next
            self._next = (self._next + 1) % self.slots
            if slot in self._pending:          # the rotation came round: its files are written before its buffers are reused
                self.finish(slot)
                earlier.remove(slot)
            t = preds.tensor
            n, T, K = len(samples), t.shape[1], t.shape[-1]
            H, W = (t.shape[2], t.shape[3]) if t.dim() == 5 else (1, t.shape[2])
            fbytes = n * T * K * H * W
            roff = (fbytes + 3) // 4 * 4
            host, dev = self._buffers(slot, roff + n * T * K * 2 * 4)
            display = display_for(preds.feature_names, self.table, self.offsets)
            out = (dev[:fbytes].view(n, T, K, H, W), dev[roff:].view(torch.float32).view(n, T, K, 2))
            ops.forecast_frames(t, std, mean, display, samples=samples, out=out)     # compute stream
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(ready)
                host.copy_(dev, non_blocking=True)                                   # one DMA: frames and ranges together
                done = torch.cuda.Event()
                done.record(self.copy_stream)
            self._done[slot] = done
            self._meta[slot] = (host, (n, T, K, H, W), roff, [runtimes[b] for b in samples], list(preds.feature_names), display)
            self._pending.append(slot)
        for s in earlier:                      # the host encodes the earlier batch while this one is on the device
            self.finish(s)
        return slot

    def finish(self, slot: int) -> List[Path]:
        if slot not in self._pending:
            return []
        self._done[slot].synchronize()
        self._pending.remove(slot)
        host, (n, T, K, H, W), roff, runtimes, names, display = self._meta[slot]
        raw = host.numpy()
        frames = raw[:n * T * K * H * W].reshape(n, T, K, H, W)
        ranges = raw[roff:roff + n * T * K * 8].view(np.float32).reshape(n, T, K, 2)
        paths = []
        for i, runtime in enumerate(runtimes):
            for k, feature in enumerate(names):
                cmap = display[k].cmap
                if cmap not in self._palettes:
                    self._palettes[cmap] = palette_for(cmap)
                path = self.settings.get_gif_path(runtime, feature)
                save_palette_gif(path, frames[i, :, k], self._palettes[cmap])
                side = {"feature": feature, "runtime": runtime, "colormap": cmap,
                        "titles": [f"{runtime} +{t + 1}h" for t in range(T)],
                        "ranges": [[None if v != v else float(v) for v in ranges[i, t, k]] for t in range(T)]}
                with open(str(path) + ".json", "w") as f:
                    json.dump(side, f)
                paths.append(path)
        self.written.extend(paths)
        return paths

    def drain(self) -> None:
        for slot in list(self._pending):
            self.finish(slot)
