"""
Output staging for the inference path: what happens between the rollout and the GRIB / GIF writers.

The reference (py4cast/lightning.py:1162-1188, py4cast/io/outputs.py:116-241) un-normalises the prediction feature by feature
on the device, then the writers pull ONE (lat, lon) plane per time step and feature with ``tensor[:, :, idx].cpu().numpy()``: a
strided gather plus a synchronous device-to-host copy per plane (3 steps x 60 features = 180 blocking copies per sample).

Here the un-normalisation kernel writes feature-major planes (``p4c_unnormalize_planes``: (B,T,*S,F) -> (B,T,F,*S), bit-exact
with the reference's two rounded steps) and the planes travel to PINNED host buffers with ONE asynchronous copy per batch on a
copy stream.  Two buffers rotate, so the next batch's rollout, the copy of this batch and the host-side writers (CPU-bound:
epygram / matplotlib) of the previous one overlap.

The GRIB writer is native (``ForecastGribWriter``): ``ops.grib_pack`` finds every field's range and packs it on the device at the
template's decimal scale factor and width (GRIB2 simple packing), params and bit streams leave with one asynchronous copy, and the
host only wraps them into the template's messages (``grib2.py``: no epygram, no eccodes); ``grib_fid`` holds the reference's key
table.  With ``packing="template"`` or ``"complex"`` (``OutputSavingSettings.grib_packing``) the fields of complex-packed template
messages go through ``ops.grib_pack_complex`` (GRIB2 templates 5.2 / 5.3) instead, in the same submit.

The GIF writer is native (``ForecastGifWriter``): ``ops.forecast_frames`` turns the normalised prediction into palette-index
frames on the device -- one byte per pixel, every feature of every lead time of the accepted samples, the reference's colour table
and range per parameter (``display_for``) -- the frames and their ranges leave with one asynchronous copy, and the host only wraps
them into "P"-mode GIF frames; no figure is drawn.  ``OutputSavingSettings`` reads the reference's io_conf JSON files.
"""

import json
from dataclasses import dataclass, fields
from datetime import datetime, timedelta
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
    grib_packing: str = "simple"        # ForecastGribWriter's ``packing``: "simple", "template" or "complex"

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

    def get_grib_path(self, runtime: str, member: int, leadtime) -> Path:
        """io/outputs.py:88-98: the identifiers ``leadtime`` and ``member`` (three digits); ``runtime`` and ``date`` name the runtime"""
        values = {"leadtime": leadtime, "member": str(member).zfill(3), "runtime": runtime, "date": runtime}
        return self._path(Path(self.dir_grib), runtime, self.grib_fmt, self.grib_identifiers, values)

    @property
    def template_path(self) -> Path:
        return Path(self.dir_grib) / self.template_grib


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


# ------------------------------------------------------------------------------------------------ forecast GRIBs
# the GRIB2 keys a feature is written with (io/outputs.py:325-433; WMO code tables 4.1, 4.2, 4.5, 4.10): Template.find compares them
GRIB_FIDS = {
    "temperature": {"editionNumber": 2, "name": "2 metre temperature", "shortName": "2t", "discipline": 0, "parameterCategory": 0,
                    "parameterNumber": 0, "typeOfFirstFixedSurface": 103, "level": 2, "typeOfSecondFixedSurface": 255,
                    "tablesVersion": 15, "productDefinitionTemplateNumber": 0},
    "u10": {"editionNumber": 2, "name": "10 metre U wind component", "shortName": "10u", "discipline": 0, "parameterCategory": 2,
            "parameterNumber": 2, "typeOfFirstFixedSurface": 103, "level": 10, "typeOfSecondFixedSurface": 255, "tablesVersion": 15,
            "productDefinitionTemplateNumber": 0},
    "v10": {"editionNumber": 2, "name": "10 metre V wind component", "shortName": "10v", "discipline": 0, "parameterCategory": 2,
            "parameterNumber": 3, "typeOfFirstFixedSurface": 103, "level": 10, "typeOfSecondFixedSurface": 255, "tablesVersion": 15,
            "productDefinitionTemplateNumber": 0},
    "r2": {"editionNumber": 2, "name": "2 metre relative humidity", "shortName": "2r", "discipline": 0, "parameterCategory": 1,
           "parameterNumber": 1, "typeOfFirstFixedSurface": 103, "level": 2, "typeOfSecondFixedSurface": 255, "tablesVersion": 15,
           "productDefinitionTemplateNumber": 0},
    "pmer": {"editionNumber": 2, "name": "Pressure reduced to MSL", "shortName": "prmsl", "discipline": 0, "parameterCategory": 3,
             "parameterNumber": 1, "typeOfFirstFixedSurface": 101, "level": 0, "typeOfSecondFixedSurface": 255, "tablesVersion": 15,
             "productDefinitionTemplateNumber": 0},
    "tp": {"editionNumber": 2, "name": "Time integral of rain flux", "shortName": "tirf", "discipline": 0, "parameterCategory": 1,
           "parameterNumber": 65, "typeOfFirstFixedSurface": 1, "level": 0, "typeOfSecondFixedSurface": 255, "tablesVersion": 15,
           "productDefinitionTemplateNumber": 8, "lengthOfTimeRange": 1, "typeOfStatisticalProcessing": 1},
}
GRIB_FEATURES = {
    "aro_t2m_2m": "temperature", "t2m_2_heightAboveGround": "temperature", "u10_10_heightAboveGround": "u10", "aro_u10_10m": "u10",
    "v10_10_heightAboveGround": "v10", "aro_v10_10m": "v10", "aro_prmsl_0hpa": "pmer", "aro_r2_2m": "r2", "aro_tp_0m": "tp",
}


def grib_fid(feature: str, time_step: int):
    """(the GRIB2 keys of a feature, its cumulative duration) as the reference's ``feature2fid`` gives them: (None, None) for a feature
    that is not written; the duration -- ``time_step`` seconds -- only for the accumulated one (precipitation), else None."""
    key = GRIB_FEATURES.get(feature)
    if key is None:
        return None, None
    return dict(GRIB_FIDS[key]), (timedelta(seconds=time_step) if key == "tp" else None)


@dataclass
class GribSample:
    """What the file names and the headers of one sample's GRIBs need (io/outputs.py:132-160)"""

    runtime: str
    basis: datetime                  # of the initial state: section 1's reference time
    terms: List[timedelta]           # one per lead time
    time_step: int                   # seconds between two steps: the cumulative duration
    member: int                      # as in the file name: the dataset's member + 1

    @classmethod
    def from_sample(cls, sample, runtime: str) -> "GribSample":
        deltas = sample.timestamps.timedeltas
        return cls(runtime, sample.output_timestamps.datetime, list(sample.output_timestamps.timedeltas),
                   int((deltas[1] - deltas[0]).total_seconds()), getattr(sample, "member") + 1)


class ForecastGribWriter:
    """One GRIB2 file per (accepted sample, lead time) of a predicted batch, one message per feature ``grib_fid`` accepts, in the
    prediction's feature order (io/outputs.py:116-220), each message the template's with new times and a new simple-packed field.

    ``submit`` enqueues ``ops.grib_pack`` on the current stream and ONE asynchronous copy of params + bit streams into a pinned
    buffer on the copy stream, then assembles what an earlier ``submit`` left pending: batch i's files are written by the host while
    batch i+1 is on the device.  ``finish(slot)`` waits for that batch's copy only; ``drain`` finishes what is pending.  On a CPU
    tensor the fields are packed by ``grib2.pack_fields`` (the same contract in numpy) and everything else is the same code.

    ``grid_lat`` / ``grid_lon``: the forecast grid, (H, W) or vectors; its place in the template's grid follows ``match_latlon``,
    the points of the template outside it are absent in the bitmap.

    ``packing``: "simple" (the default) writes every field in simple packing (template 5.0) whatever the template message is packed
    with; "template" follows each template message -- 5.0: simple; 5.2: complex packing; 5.3: complex packing with spatial
    differencing of the message's order (octet 48) --; "complex" writes 5.3 at order 2 for every feature.  Complex-packed fields go
    through ``ops.grib_pack_complex`` (``grib2.pack_fields`` on the CPU) in the same submit; a feature whose width leaves the limits
    of that route (nbits + order <= 31) is written in 5.0, with one warning.  The complex streams' length is known on the device
    only, so such a submit makes two copies: the params first and, once they are on the host -- after the earlier batch's files are
    written --, exactly the bytes up to the end of the last payload."""

    PACKINGS = ("simple", "template", "complex")

    def __init__(self, settings: OutputSavingSettings, device: torch.device, grid_lat, grid_lon, template=None, slots: int = 2,
                 packing: str = "simple"):
        from . import grib2

        if packing not in self.PACKINGS:
            raise ValueError(f"packing {packing!r}: one of {self.PACKINGS}")
        self.packing = packing
        self._warned_limits = False
        self.copied: Optional[Tuple[int, int]] = None   # the bytes of the last mixed submit's two copies: params, streams
        self.settings, self.device, self.slots = settings, torch.device(device), slots
        self.template = grib2.Template(settings.template_path) if template is None else template
        self.grid_lat, self.grid_lon = np.asarray(grid_lat, dtype=np.float64), np.asarray(grid_lon, dtype=np.float64)
        self.copy_stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None
        self._host: List[Optional[torch.Tensor]] = [None] * slots
        self._dev: List[Optional[torch.Tensor]] = [None] * slots
        self._done = [None] * slots
        self._meta = [None] * slots
        self._pending: List[int] = []
        self._next = 0
        self._plans: Dict[tuple, tuple] = {}
        self.written: List[Path] = []          # every file written so far, in order

    @classmethod
    def for_dataset(cls, settings: OutputSavingSettings, infer_ds, device) -> Optional["ForecastGribWriter"]:
        """The writer of an inference dataset, or None when something it needs is missing: the settings' template file (it must exist
        and parse), ``infer_ds.sample_list`` (dates, terms, member) or ``infer_ds.grid`` (``lat``, ``lon``)."""
        from . import grib2

        grid = getattr(infer_ds, "grid", None)
        if getattr(infer_ds, "sample_list", None) is None or getattr(grid, "lat", None) is None or getattr(grid, "lon", None) is None:
            return None
        if not settings.template_path.is_file():
            return None
        try:
            template = grib2.Template(settings.template_path)
        except (grib2.GribError, OSError):
            return None
        return cls(settings, device, grid.lat, grid.lon, template=template, packing=settings.grib_packing)

    def _buffers(self, slot: int, nbytes: int):
        if self._host[slot] is None or self._host[slot].numel() < nbytes:
            self._host[slot] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            self._dev[slot] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._host[slot][:nbytes], self._dev[slot][:nbytes]

    def _order(self, m, name: str, nbits: int) -> Optional[int]:
        """None: the feature is written in simple packing; 0, 1, 2: in complex packing at that order"""
        import warnings

        from . import grib2

        if self.packing == "simple":
            return None
        order = 2 if self.packing == "complex" else grib2.packing_of(m)
        if order and nbits + order > 31:
            if not self._warned_limits:
                self._warned_limits = True
                warnings.warn(f"{name}: {nbits} bits at order {order} leave the limits of the complex packing written here "
                              f"(nbits + order <= 31); such features are written in simple packing (5.0)")
            return None
        return order

    def _plan(self, names: tuple, H: int, W: int):
        """(feature indices, template messages, (D, nbits) each, window, flip_rows, the order of the complex packing or None each) of a
        prediction with these feature names"""
        from . import grib2

        key = (names, H, W)
        if key not in self._plans:
            index, messages, spec, orders = [], [], [], []
            for f, name in enumerate(names):
                fid, _ = grib_fid(name, 0)
                if fid is None:
                    continue
                m = self.template.find(fid)
                grib2.check_product(m)
                index.append(f)
                messages.append(m)
                spec.append(grib2.spec_of(m))
                orders.append(self._order(m, name, spec[-1][1]))
            window, flip = None, False
            if messages:
                if any(m.sections[3] != messages[0].sections[3] for m in messages):
                    raise ValueError(f"{self.template.path}: the messages of the written features are not on one grid")
                Ni, Nj, lat, lon, _ = grib2.grid_of(messages[0])
                window = grib2.match_latlon(self.grid_lat, self.grid_lon, lat, lon)
                if (window[1] - window[0] + 1, window[3] - window[2] + 1) != (H, W):
                    raise ValueError("Lat/Lon dims of the dataset do not fit in template grid, cannot write grib.")
                column = self.grid_lat[:, 0] if self.grid_lat.ndim == 2 else self.grid_lat.reshape(-1)
                # the stream follows the template's rows: flipped when it runs north to south over a grid whose row 0 is the southern one
                flip = bool(H > 1 and (column[-1] > column[0]) != (lat[-1] > lat[0]))
            self._plans[key] = (tuple(index), messages, spec, window, flip, orders)
        return self._plans[key]

    def submit(self, preds: NamedTensor, std: torch.Tensor, mean: torch.Tensor, samples: Sequence[Optional[GribSample]]) -> Optional[int]:
        """preds: the NORMALISED prediction (B,T,H,W,F); ``samples[b]``: sample b's GribSample, or None when it is not written.
        Returns the slot for ``finish``, or None when nothing is to be written (nothing is launched)."""
        from . import grib2

        accepted = [b for b, s in enumerate(samples) if s is not None]
        earlier = list(self._pending)
        slot = None
        t = preds.tensor
        H, W = (t.shape[2], t.shape[3]) if t.dim() == 5 else (1, t.shape[2])
        index, messages, spec, window, flip, orders = self._plan(tuple(preds.feature_names), H, W) if accepted \
            else ((), [], [], None, False, [])
        second_copy = None
        if accepted and index and any(o is not None for o in orders):
            slot, second_copy = self._submit_mixed(preds, std, mean, samples, accepted, earlier)
        elif accepted and index:
            slot = self._next
            self._next = (self._next + 1) % self.slots
            if slot in self._pending:          # the rotation came round: its files are written before its buffers are reused
                self.finish(slot)
                earlier.remove(slot)
            n, T, K, N = len(accepted), t.shape[1], len(index), H * W
            pitch = ops.grib_pitch(N, spec)
            pbytes = n * T * K * ops.GRIB_PARAMS * 4
            if t.is_cuda:
                host, dev = self._buffers(slot, pbytes + n * T * K * pitch)
                out = (dev[:pbytes].view(torch.int32).view(n, T, K, ops.GRIB_PARAMS), dev[pbytes:].view(n, T, K, pitch))
                ops.grib_pack(t, std, mean, spec, samples=accepted, features=index, flip_rows=flip, out=out)   # compute stream
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(self.copy_stream):
                    self.copy_stream.wait_event(ready)
                    host.copy_(dev, non_blocking=True)                                # one DMA: params and streams together
                    done = torch.cuda.Event()
                    done.record(self.copy_stream)
                self._done[slot] = done
                raw = host.numpy()
                params, packed = raw[:pbytes].view(np.int32).reshape(n, T, K, ops.GRIB_PARAMS), raw[pbytes:].reshape(n, T, K, pitch)
            else:
                x = t.detach().float().reshape(t.shape[0], T, N, t.shape[-1]).numpy()
                params, packed = grib2.pack_fields(x, std.detach().float().numpy(), mean.detach().float().numpy(), spec, accepted, index,
                                                   H, W, flip, pitch)
                self._done[slot] = None
            self._meta[slot] = (params, packed, N, [samples[b] for b in accepted], [preds.feature_names[f] for f in index], messages,
                                spec, window, None)
            self._pending.append(slot)
        for s in earlier:                      # the host writes the earlier batch while this one is on the device
            self.finish(s)
        if second_copy is not None:
            second_copy()
        return slot

    def _submit_mixed(self, preds, std, mean, samples, accepted, earlier):
        """``submit`` with complex-packed features: the simple-packed ones (if any) and the complex-packed ones go through one call
        each, the params of both are copied at once.  -> (slot, what ``submit`` runs after the earlier batch's files are written: it
        waits for the params and enqueues the copy of the streams, sized by the last payload's end; None on the CPU)"""
        from . import grib2

        t = preds.tensor
        H, W = (t.shape[2], t.shape[3]) if t.dim() == 5 else (1, t.shape[2])
        index, messages, spec, window, flip, orders = self._plan(tuple(preds.feature_names), H, W)
        slot = self._next
        self._next = (self._next + 1) % self.slots
        if slot in self._pending:
            self.finish(slot)
            earlier.remove(slot)
        n, T, N = len(accepted), t.shape[1], H * W
        ks = [k for k, o in enumerate(orders) if o is None]          # written in simple packing
        kc = [k for k, o in enumerate(orders) if o is not None]      # in complex packing
        spec_s, spec_c = [spec[k] for k in ks], [(spec[k][0], spec[k][1], orders[k]) for k in kc]
        index_s, index_c = [index[k] for k in ks], [index[k] for k in kc]
        pitch = ops.grib_pitch(N, spec_s) if ks else 0
        words_s, words_c = n * T * len(ks) * ops.GRIB_PARAMS, n * T * len(kc) * ops.GRIB_COMPLEX_PARAMS
        pbytes, sbytes = 4 * (words_s + words_c), n * T * len(ks) * pitch
        capacity = ops.grib_complex_capacity(n, T, N, spec_c)
        shape_s, shape_c = (n, T, len(ks), ops.GRIB_PARAMS), (n, T, len(kc), ops.GRIB_COMPLEX_PARAMS)
        second_copy = None
        if t.is_cuda:
            host, dev = self._buffers(slot, pbytes + sbytes + capacity)
            if ks:
                ops.grib_pack(t, std, mean, spec_s, samples=accepted, features=index_s, flip_rows=flip,
                              out=(dev[:4 * words_s].view(torch.int32).view(shape_s), dev[pbytes:pbytes + sbytes].view(n, T, len(ks), pitch)))
            ops.grib_pack_complex(t, std, mean, spec_c, samples=accepted, features=index_c, flip_rows=flip,
                                  out=(dev[4 * words_s:pbytes].view(torch.int32).view(shape_c), dev[pbytes + sbytes:]))
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(ready)
                host[:pbytes].copy_(dev[:pbytes], non_blocking=True)                  # copy 1: the params of both calls
                have_params = torch.cuda.Event()
                have_params.record(self.copy_stream)
            self._done[slot] = have_params
            raw = host.numpy()
            params_c = raw[4 * words_s:pbytes].view(np.int32).reshape(shape_c)

            def second_copy():
                have_params.synchronize()
                last = params_c.reshape(-1, ops.GRIB_COMPLEX_PARAMS)[-1]
                used = sbytes + int(last[10]) + int(last[9])                          # copy 2: up to the end of the last payload
                with torch.cuda.stream(self.copy_stream):
                    if used:
                        host[pbytes:pbytes + used].copy_(dev[pbytes:pbytes + used], non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(self.copy_stream)
                self._done[slot] = done
                self.copied = (pbytes, used)

            params_s = raw[:4 * words_s].view(np.int32).reshape(shape_s)
            packed = raw[pbytes:pbytes + sbytes].reshape(n, T, len(ks), pitch)
            stream = raw[pbytes + sbytes:]
        else:
            x = t.detach().float().reshape(t.shape[0], T, N, t.shape[-1]).numpy()
            sd, mu = std.detach().float().numpy(), mean.detach().float().numpy()
            params_s, packed = grib2.pack_fields(x, sd, mu, spec_s, accepted, index_s, H, W, flip, pitch) if ks else (None, None)
            params_c, stream = grib2.pack_fields(x, sd, mu, spec_c, accepted, index_c, H, W, flip)
            self._done[slot] = None
        self._meta[slot] = (params_s, packed, N, [samples[b] for b in accepted], [preds.feature_names[f] for f in index], messages, spec,
                            window, (orders, params_c, stream))
        self._pending.append(slot)
        return slot, second_copy

    def finish(self, slot: int) -> List[Path]:
        import warnings

        from . import grib2

        if slot not in self._pending:
            return []
        if self._done[slot] is not None:
            self._done[slot].synchronize()
        self._pending.remove(slot)
        params, packed, N, samples, names, messages, spec, window, mixed = self._meta[slot]
        if mixed is not None:
            return self._finish_mixed(slot)
        reals = params[..., :3].view(np.float32)
        paths = []
        for i, sample in enumerate(samples):
            for t, term in enumerate(sample.terms):
                path = self.settings.get_grib_path(sample.runtime, sample.member, int(term.total_seconds() / 60 ** 2))
                with open(path, "wb") as f:
                    for k, name in enumerate(names):
                        if params[i, t, k, 4]:
                            warnings.warn(f"{path}: {name} holds {int(params[i, t, k, 4])} values that are not finite; the field is not written")
                            continue
                        D, nbits = spec[k]
                        f.write(grib2.encode(messages[k], sample.basis, term, cumulative=grib_fid(name, sample.time_step)[1], window=window,
                                             packed=packed[i, t, k, :(N * nbits + 7) // 8].tobytes(), R=float(reals[i, t, k, 2]),
                                             E=int(params[i, t, k, 3]), D=D, nbits=nbits))
                paths.append(path)
        self.written.extend(paths)
        return paths

    def _finish_mixed(self, slot: int) -> List[Path]:
        """the files of a batch with complex-packed features: message k from the simple or from the complex call's output"""
        import warnings

        from . import grib2

        params_s, packed, N, samples, names, messages, spec, window, (orders, params_c, stream) = self._meta[slot]
        place, ns, nc = [], 0, 0                      # feature k -> its index in its call
        for o in orders:
            place.append(ns if o is None else nc)
            ns, nc = ns + (o is None), nc + (o is not None)
        paths = []
        for i, sample in enumerate(samples):
            for t, term in enumerate(sample.terms):
                path = self.settings.get_grib_path(sample.runtime, sample.member, int(term.total_seconds() / 60 ** 2))
                with open(path, "wb") as f:
                    for k, name in enumerate(names):
                        rec = (params_s if orders[k] is None else params_c)[i, t, place[k]]
                        if rec[4]:
                            warnings.warn(f"{path}: {name} holds {int(rec[4])} values that are not finite; the field is not written")
                            continue
                        D, nbits = spec[k]
                        common = dict(cumulative=grib_fid(name, sample.time_step)[1], window=window, R=float(rec[2:3].view(np.float32)[0]),
                                      E=int(rec[3]), D=D, nbits=nbits)
                        if orders[k] is None:
                            f.write(grib2.encode(messages[k], sample.basis, term, packed=packed[i, t, place[k], :(N * nbits + 7) // 8].tobytes(),
                                                 **common))
                        else:
                            f.write(grib2.encode(messages[k], sample.basis, term, packed=stream[int(rec[10]):int(rec[10]) + int(rec[9])].tobytes(),
                                                 order=orders[k], ref_bits=int(rec[8]), **common))
                paths.append(path)
        self.written.extend(paths)
        return paths

    def drain(self) -> None:
        for slot in list(self._pending):
            self.finish(slot)
