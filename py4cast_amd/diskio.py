"""
On-disk formats either side of the hot path, host side.

* Titan's training layout: one 2-D ``.npy`` plane per (date, parameter) --
  ``<dataset>/data/<date %Y-%m-%d_%Hh%M>/<name>_<level><hpa|m>.npy`` (datasets/titan/__init__.py:93-109,168-176), read by
  ``np.load`` per plane (:111-129), stacked per parameter and standardised on the CPU (datasets/base.py:431-453).
  Here the planes of a whole batch are read straight into ONE pinned host buffer (the ``.npy`` payload is ``readinto`` its slot:
  no intermediate arrays), copied to the device in one asynchronous transfer and standardised + packed into the features-last
  batch by one kernel (``datapipe.standardize_and_collate`` -> ``p4c_pack_standardize``).
* Statistics files: ``parameters_stats.pt`` / ``diff_stats.pt`` = ``torch.save`` of ``{name: {"mean","std","min","max": 0-d
  tensor}}`` (datasets/compute_dataset_stats.py:71-127, read by ``Stats`` at datasets/access.py:355-390, written by the dummy
  dataset at datasets/dummy.py:24-42).
* Titan's GRIB layout (``file_format="grib"``, the reference's default: datasets/titan/__init__.py:112-152): ``GribPlaneReader``
  ships the packed bit streams of a batch as they lie in the files and ``ops.grib_unpack`` decodes them on the device.
  ``decode_placed`` is its device half, ``GribFileCache`` the parsed files shared by the loader's threads (``datasets.GribRoutes``),
  ``convert_titan_grib_to_npy`` the conversion to the ``.npy`` layout above.
"""

import datetime as dt
import os
from collections import OrderedDict
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from numpy.lib import format as npy_format

from .base import Stats

TITAN_FORMATSTR = "%Y-%m-%d_%Hh%M"   # datasets/titan/settings.py:8


# ------------------------------------------------------------------------------------------ statistics files
def save_stats(stats: Dict[str, Dict[str, torch.Tensor]], fname) -> None:
    """The reference's layout: dict of dict of 0-d tensors, ``torch.save`` (compute_dataset_stats.py:84-85,126-127)."""
    out = {name: {k: torch.as_tensor(v).detach().cpu().reshape(()) for k, v in d.items()} for name, d in stats.items()}
    torch.save(out, fname)


def load_stats(fname) -> Stats:
    """``Stats(fname)`` of the reference (access.py:355-362)."""
    return Stats(torch.load(fname, "cpu", weights_only=True))


def write_dataset_stats(dataset, cache_dir, device=None) -> Tuple[Path, Path]:
    """compute_dataset_stats.py end to end on the device kernels, as the accessors' ``prepare`` runs it (datasets/rainfall.py:196-246):
    ``parameters_stats.pt`` on the raw values (``settings.standardize`` off), then ``diff_stats.pt`` on values standardised with the
    file just written (``settings.standardize`` on; pass the dataset's own ``cache_dir`` so that it is the file the dataset reads).
    The dataset's setting is put back afterwards."""
    from . import dataset_stats as ds

    cache_dir = Path(cache_dir)
    os.makedirs(cache_dir, exist_ok=True)
    p1, p2 = cache_dir / "parameters_stats.pt", cache_dir / "diff_stats.pt"
    keep = dataset.settings.standardize
    try:
        dataset.settings.standardize = False
        save_stats(ds.compute_parameters_stats(dataset, device), p1)
        dataset.settings.standardize = True
        getattr(dataset, "__dict__", {}).pop("stats", None)      # a cached Stats of an earlier file
        save_stats(ds.compute_time_step_stats(dataset, device), p2)
    finally:
        dataset.settings.standardize = keep
    return p1, p2


# ------------------------------------------------------------------------------------------ .npy planes
def titan_plane_path(dataset_path, name: str, level: int, level_type: str, date: dt.datetime) -> Path:
    """datasets/titan/__init__.py:93-109 (npy branch) with parameter_namer (:168-176)."""
    suffix = "m" if level_type in ("surface", "heightAboveGround") else "hpa"
    return Path(dataset_path) / "data" / date.strftime(TITAN_FORMATSTR) / f"{name}_{level}{suffix}.npy"


def _read_header(f):
    version = npy_format.read_magic(f)
    if version == (1, 0):
        shape, fortran, dtype = npy_format.read_array_header_1_0(f)
    elif version == (2, 0):
        shape, fortran, dtype = npy_format.read_array_header_2_0(f)
    else:
        raise ValueError(f"unsupported .npy version {version}")
    return shape, fortran, dtype


class NpyPlaneReader:
    """Reads (F, B, T) planes of H x W values into one pinned host buffer and returns them on the device as the
    (F, B, T, H, W) fp32 tensor ``datapipe.standardize_and_collate`` consumes."""

    def __init__(self, shape: Tuple[int, int], n_features: int, batch: int, steps: int, device=None, pin: Optional[bool] = None):
        self.shape = tuple(shape)
        self.dims = (n_features, batch, steps)
        self.device = device
        pin = torch.cuda.is_available() if pin is None else pin
        self.host = torch.empty(n_features, batch, steps, *self.shape, dtype=torch.float32, pin_memory=pin)
        self._np = self.host.numpy()     # same memory
        self.copy_stream = torch.cuda.Stream(device) if (device is not None and torch.device(device).type == "cuda") else None

    def _read_plane(self, path, dst: np.ndarray) -> None:
        with open(path, "rb") as f:
            shape, fortran, dtype = _read_header(f)
            if tuple(shape) != self.shape:
                raise ValueError(f"{path}: plane shape {tuple(shape)} != {self.shape}")
            if fortran:
                raise ValueError(f"{path}: Fortran-ordered planes are not supported")
            if dtype == np.dtype("<f4"):
                n = f.readinto(memoryview(dst).cast("B"))    # payload straight into the pinned slot
                if n != dst.nbytes:
                    raise ValueError(f"{path}: truncated file ({n} of {dst.nbytes} bytes)")
            else:                                            # other dtypes: numpy converts (np.load + astype in the reference's terms)
                dst[...] = np.fromfile(f, dtype=dtype, count=int(np.prod(shape))).reshape(shape).astype(np.float32)

    def read(self, paths: Sequence[Sequence[Sequence]]) -> torch.Tensor:
        """paths[f][b][t] -> (F, B, T, H, W) tensor on ``device`` (or the host buffer itself when device is None)."""
        F, B, T = self.dims
        if len(paths) != F or any(len(pb) != B or any(len(pt) != T for pt in pb) for pb in paths):
            raise ValueError(f"expected paths[{F}][{B}][{T}]")
        for fi in range(F):
            for b in range(B):
                for t in range(T):
                    self._read_plane(paths[fi][b][t], self._np[fi, b, t])
        if self.device is None:
            return self.host
        if self.copy_stream is None:
            return self.host.to(self.device)
        self.copy_stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.copy_stream):
            dev = self.host.to(self.device, non_blocking=True)
        torch.cuda.current_stream(self.device).wait_stream(self.copy_stream)   # the consumer kernel runs after the transfer
        dev.record_stream(torch.cuda.current_stream(self.device))
        return dev


def load_titan_batch(dataset_path, params: List[Tuple[str, int, str]], dates: List[List[dt.datetime]], stats: Stats,
                     num_input_steps: int, forcing, reader: Optional[NpyPlaneReader] = None, device=None, standardize: bool = True):
    """``Sample.load`` + ``collate_fn`` for the input_output parameters of a batch read from Titan's .npy layout.
    params: (name, level, level_type); dates[b][t]: validity times of sample b.  Returns an ItemBatch on ``device``."""
    from . import datapipe

    B, T = len(dates), len(dates[0])
    paths = [[[titan_plane_path(dataset_path, n, lv, lt, dates[b][t]) for t in range(T)] for b in range(B)] for (n, lv, lt) in params]
    if reader is None:
        with open(paths[0][0][0], "rb") as f:
            shape, _, _ = _read_header(f)
        reader = NpyPlaneReader(shape, len(params), B, T, device=device)
    raw = reader.read(paths)
    names = [f"{n}_{lv}{'m' if lt in ('surface', 'heightAboveGround') else 'hpa'}" for (n, lv, lt) in params]
    return datapipe.load_batch(raw, names, forcing, stats, num_input_steps, standardize)


class TypedNpyPlaneReader:
    """``NpyPlaneReader`` for planes that are NOT ``<f4`` (which that reader converts on the host): the payloads go into the pinned
    buffer in the files' own dtype ``dtype`` (u8, i16, u16, i32, f16, f32, f64) and ``read`` returns the typed (F, B, T, H, W) device
    tensor ``datapipe.load_typed_batch`` consumes -- the conversion happens in ``p4c_pack_convert``.  Every feature's block of B x T
    planes starts on a 16-byte boundary (the tensor is a view with that pitch between features)."""

    def __init__(self, shape: Tuple[int, int], dtype, n_features: int, batch: int, steps: int, device=None, pin: Optional[bool] = None):
        self.shape, self.dtype, self.dims, self.device = tuple(shape), np.dtype(dtype), (n_features, batch, steps), device
        H, W = self.shape
        self.block = (batch * steps * H * W * self.dtype.itemsize + 15) // 16 * 16
        pin = torch.cuda.is_available() if pin is None else pin
        self.host = torch.empty(max(self.block * n_features, 16), dtype=torch.uint8, pin_memory=pin)
        per = self.block // self.dtype.itemsize
        self._strides = (per, steps * H * W, H * W, W, 1)
        self._np = np.lib.stride_tricks.as_strided(self.host.numpy().view(self.dtype), (n_features, batch, steps, H, W),
                                                   tuple(v * self.dtype.itemsize for v in self._strides), writeable=True)
        self.copy_stream = torch.cuda.Stream(device) if (device is not None and torch.device(device).type == "cuda") else None
        self._copied = None     # the event behind the last copy out of ``host``: the buffer is refilled only after it

    def _typed(self, flat: torch.Tensor) -> torch.Tensor:
        tdtype = torch.uint16 if self.dtype == np.uint16 else torch.from_numpy(np.zeros(0, dtype=self.dtype)).dtype
        return flat.view(tdtype).as_strided((*self.dims, *self.shape), self._strides)

    def read(self, paths: Sequence[Sequence[Sequence]]) -> torch.Tensor:
        """paths[f][b][t] -> (F, B, T, H, W) tensor of the files' dtype on ``device`` (a view of the host buffer when it is None)"""
        F, B, T = self.dims
        if len(paths) != F or any(len(pb) != B or any(len(pt) != T for pt in pb) for pb in paths):
            raise ValueError(f"expected paths[{F}][{B}][{T}]")
        if self._copied is not None:
            self._copied.synchronize()          # the last call's copy has left the buffer
            self._copied = None
        for fi in range(F):
            for b in range(B):
                for t in range(T):
                    dst = self._np[fi, b, t]
                    with open(paths[fi][b][t], "rb") as f:
                        shape, fortran, dtype = _read_header(f)
                        if tuple(shape) != self.shape or fortran or np.dtype(dtype) != self.dtype:
                            raise ValueError(f"{paths[fi][b][t]}: holds {tuple(shape)} {dtype}{' (Fortran order)' if fortran else ''}, "
                                             f"expected {self.shape} {self.dtype}")
                        n = f.readinto(memoryview(dst).cast("B"))
                        if n != dst.nbytes:
                            raise ValueError(f"{paths[fi][b][t]}: truncated file ({n} of {dst.nbytes} bytes)")
        if self.device is None or self.copy_stream is None:
            return self._typed(self.host if self.device is None else self.host.to(self.device))
        current = torch.cuda.current_stream(self.device)
        self.copy_stream.wait_stream(current)
        with torch.cuda.stream(self.copy_stream):
            dev = self.host.to(self.device, non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record(self.copy_stream)
        current.wait_stream(self.copy_stream)
        dev.record_stream(current)
        return self._typed(dev)


def load_titan_typed_batch(dataset_path, params: List[Tuple[str, int, str]], dates: List[List[dt.datetime]], stats: Stats,
                           num_input_steps: int, forcing, reader: Optional[TypedNpyPlaneReader] = None, device=None,
                           standardize: bool = True, transforms=None, host: bool = False):
    """``load_titan_batch`` for ``.npy`` planes of any dtype ``p4c_pack_convert`` reads, all of one dtype: no conversion on the host.
    transforms: as ``datapipe.load_typed_batch`` takes them (None: the planes are standardised as they are).  Without a CUDA
    ``device`` (or a reader on one) the call is refused -- no CPU fallback -- unless ``host=True`` asks for the numpy statement."""
    from . import datapipe

    B, T = len(dates), len(dates[0])
    paths = [[[titan_plane_path(dataset_path, n, lv, lt, dates[b][t]) for t in range(T)] for b in range(B)] for (n, lv, lt) in params]
    if reader is None:
        with open(paths[0][0][0], "rb") as f:
            shape, _, dtype = _read_header(f)
        reader = TypedNpyPlaneReader(shape, dtype, len(params), B, T, device=device)
    raw = reader.read(paths)
    names = [f"{n}_{lv}{'m' if lt in ('surface', 'heightAboveGround') else 'hpa'}" for (n, lv, lt) in params]
    return datapipe.load_typed_batch(raw, names, transforms, forcing, stats, num_input_steps, standardize, host)


# ------------------------------------------------------------------------------------------ GRIB2 files
def titan_grib_path(dataset_path, grib_name: str, date: dt.datetime) -> Path:
    """datasets/titan/__init__.py:93-109 (grib branch): ``<dataset>/grib/<date>/<grib_name>``."""
    return Path(dataset_path) / "grib" / date.strftime(TITAN_FORMATSTR) / grib_name


def decode_placed(dev: torch.Tensor, chosen, where, pitch: int, check: bool = True):
    """The device half of ``GribPlaneReader.read``: ``chosen[i]`` = (path, message, field) whose stream and bitmap lie in the device
    byte buffer ``dev`` at ``where[i]`` = (stream_off, bitmap_off; -1 without a bitmap) -> (flat fp32 tensor with plane i at
    ``i * pitch`` floats, the status words of the complex-packed fields or None).  ``ops.grib_unpack`` decodes the simple-packed
    fields, ``ops.grib_unpack_complex`` the others; ``check`` copies the status words back and raises ``grib2.GribError`` naming the
    file and the condition."""
    from . import grib2, ops

    # plane i of the output belongs to chosen[i], whichever of the two tables it is decoded from
    simple = [i for i, (_, _, f) in enumerate(chosen) if not isinstance(f, grib2.ComplexField)]
    packed = [i for i, (_, _, f) in enumerate(chosen) if isinstance(f, grib2.ComplexField)]
    table = np.zeros(len(simple), dtype=ops.GRIB_FIELD)
    for j, i in enumerate(simple):
        _, _, f = chosen[i]
        s_off, b_off = where[i]
        table[j] = (s_off, len(f.stream), b_off, i * pitch, f.ni, f.nj, f.count, f.nbits, f.E, f.D, f.R, int(f.south_to_north), 0, 0)
    ctable = np.zeros(len(packed), dtype=ops.GRIB_CFIELD)
    for j, i in enumerate(packed):
        _, _, f = chosen[i]
        rec = ctable[j]
        rec["stream_off"], rec["bitmap_off"] = where[i]
        rec["stream_len"], rec["dst_off"], rec["flip_rows"] = len(f.stream), i * pitch, int(f.south_to_north)
        for name in ("ni", "nj", "count", "ng", "ref_bits", "w_ref", "w_bits", "l_ref", "l_inc", "l_last", "l_bits", "order", "nbytes",
                     "ival1", "ival2", "gmin", "E", "D", "R"):
            rec[name] = getattr(f, name)
    status = None
    with torch.cuda.device(dev.device):
        flat = torch.empty(len(chosen) * pitch, dtype=torch.float32, device=dev.device)
        if simple:
            ops.grib_unpack(dev, table, out=flat)
        if packed:
            _, status = ops.grib_unpack_complex(dev, ctable, out=flat)
    if packed and check:
        # one blocking copy of len(packed) ints: the price of naming a malformed file here instead of handing on a NaN plane
        for j, st in enumerate(status.cpu().tolist()):
            if st:
                what = [text for bit, text in ((ops.GRIB_STATUS_LENGTHS, "the group lengths do not sum to the number of values"),
                                               (ops.GRIB_STATUS_WIDTH, "a group width above 32 bits"),
                                               (ops.GRIB_STATUS_STREAM, "the values need more bits than section 7 holds")) if st & bit]
                raise grib2.GribError(f"{chosen[packed[j]][0]}: complex-packed message {chosen[packed[j]][1]!r}: {'; '.join(what)}")
    return flat, status


class GribFileCache:
    """Parsed ``grib2.GribFile``s shared by reader threads: an LRU of ``cache`` files behind a lock (the reference's ``read_grib``
    keeps 50).  Two threads that ask for one new file at once may both parse it; one result is kept."""

    def __init__(self, cache: int = 50):
        import threading

        self.cache, self.files, self.lock, self.parsed = max(int(cache), 1), OrderedDict(), threading.Lock(), 0

    def peek(self, path):
        """the parsed file when the cache holds it (now its most recent one), else None: nothing is read"""
        with self.lock:
            f = self.files.get(str(path))
            if f is not None:
                self.files.move_to_end(str(path))
            return f

    def get(self, path):
        from . import grib2

        key = str(path)
        with self.lock:
            if key in self.files:
                self.files.move_to_end(key)
                return self.files[key]
        parsed = grib2.GribFile(path)
        with self.lock:
            self.parsed += 1
            f = self.files.setdefault(key, parsed)
            self.files.move_to_end(key)
            while len(self.files) > self.cache:
                self.files.popitem(last=False)
        return f


class GribPlaneReader:
    """Reads (F, B, T) fields out of GRIB2 files and returns ``(planes (F, B, T, Nj, Ni) fp32, lat (Nj,), lon (Ni,))``.

    On a device the packed bit streams and bitmaps of all selected messages are copied, as they lie in the files, into one pinned
    byte buffer at 4-byte aligned offsets (grown when needed; a message selected twice is copied once), shipped in one non-blocking
    copy on a copy stream and decoded by ``ops.grib_unpack`` (simple packing, template 5.0) and ``ops.grib_unpack_complex`` (complex
    packing, 5.2 / 5.3; a call may mix them): no value is computed on the host.  With ``device=None`` the planes are
    ``grib2.unpack_fields`` of the same fields, on the host.  An absent point (bitmap) is NaN.

    Whether the stream of a complex-packed message agrees with its header shows on the device only (``ops.GRIB_STATUS_*``).
    ``check=True``: after a call that held such messages the reader copies their status words back -- one blocking copy -- and raises
    ``grib2.GribError`` naming the file and the condition, as the host path does.  ``check=False``: no synchronisation; the words stay
    in ``last_status`` (device, one per complex-packed field in the order of the selection; None after a call without any) and a
    malformed field is an all-NaN plane.

    Plane row 0 is the NORTHERNMOST row and ``lat`` descends, whichever way the file scans: a file whose rows run south to north
    (scanning-mode bit 0x40) is flipped while it is decoded (``flip_rows``).  This is a deliberate difference from the reference,
    which flips unconditionally after ``fit_to_grid`` (datasets/titan/__init__.py:211-226) and would turn such a file upside down;
    ``datapipe.load_native_batch`` applies that flip to north-first planes.

    Messages are selected by the numeric keys of ``grib2.MATCHED_KEYS`` (``outputs.grib_fid``), not by ``shortName``.  All fields of
    one call must lie on one grid.  ``cache``: how many parsed files are kept (the reference's ``read_grib`` keeps 50)."""

    def __init__(self, device=None, pin: Optional[bool] = None, cache: int = 50, check: bool = True):
        self.device = device
        self.check = bool(check)
        self.last_status: Optional[torch.Tensor] = None   # the status words of the last call's complex-packed fields, on the device
        self.cuda = device is not None and torch.device(device).type == "cuda"
        self.pin = (torch.cuda.is_available() and self.cuda) if pin is None else pin
        self.cache = int(cache)
        self.files: "OrderedDict[str, object]" = OrderedDict()
        self.host: Optional[torch.Tensor] = None
        self.copy_stream = torch.cuda.Stream(device) if self.cuda else None
        self._copied = None     # the event behind the last copy out of ``host``
        self.parsed = 0         # files parsed so far (a cache hit does not count)

    def file(self, path):
        from . import grib2

        key = str(path)
        if key in self.files:
            self.files.move_to_end(key)
            return self.files[key]
        f = grib2.GribFile(path)
        self.parsed += 1
        self.files[key] = f
        while len(self.files) > max(self.cache, 1):
            self.files.popitem(last=False)
        return f

    def _select(self, selections):
        from . import grib2

        F = len(selections)
        B = len(selections[0]) if F else 0
        T = len(selections[0][0]) if B else 0
        if not F or not B or not T or any(len(sb) != B or any(len(st) != T for st in sb) for sb in selections):
            raise ValueError("GribPlaneReader: expected selections[F][B][T] of (path, fid), none of the three empty")
        chosen, grid, first = [], None, None
        for sf in selections:
            for sb in sf:
                for path, fid in sb:
                    m, field = self.file(path).field(fid)
                    ni, nj, lat, lon, _ = grib2.grid_of(m)
                    lat = lat[::-1] if field.south_to_north else lat
                    if grid is None:
                        grid, first = (ni, nj, lat, lon), path
                    elif (ni, nj) != grid[:2] or not (np.array_equal(np.round(lat, 5), np.round(grid[2], 5))
                                                      and np.array_equal(np.round(lon, 5), np.round(grid[3], 5))):
                        raise ValueError(f"GribPlaneReader: {path} is on a grid of {nj} x {ni} from ({lat[0]:.5f}, {lon[0]:.5f}), {first} on "
                                         f"{grid[1]} x {grid[0]} from ({grid[2][0]:.5f}, {grid[3][0]:.5f}): one call reads one grid")
                    chosen.append((str(path), m, field))
        return (F, B, T), chosen, grid

    def read(self, selections: Sequence[Sequence[Sequence]]):
        """selections[f][b][t] = (path, fid) -> (planes (F, B, T, Nj, Ni), lat (Nj,) descending, lon (Ni,)): planes on ``device``, or a
        host tensor when it is None.  On a device every plane is dense and starts at a multiple of 4 floats (16-byte stores): where
        Nj * Ni is no multiple of 4 the tensor is a view with that pitch between planes, not contiguous."""
        from . import grib2

        (F, B, T), chosen, (ni, nj, lat, lon) = self._select(selections)
        if not self.cuda:
            planes = []
            for path, _, f in chosen:
                try:
                    planes += grib2.unpack_fields([f], flip=f.south_to_north)
                except grib2.GribError as e:
                    raise grib2.GribError(f"{path}: {e}") from None
            host = torch.from_numpy(np.stack(planes).reshape(F, B, T, nj, ni))
            return (host if self.device is None else host.to(self.device)), lat.copy(), lon.copy()
        # where every distinct message's stream and bitmap go in the byte buffer, simple- and complex-packed alike
        place, at = {}, 0
        for path, m, f in chosen:
            if (path, id(m)) not in place:
                s_off, at = at, at + (len(f.stream) + 3) // 4 * 4
                b_off = -1
                if f.bitmap is not None:
                    b_off, at = at, at + (len(f.bitmap) + 3) // 4 * 4
                place[path, id(m)] = (s_off, b_off, f)
        if self._copied is not None:
            self._copied.synchronize()          # the last call's copy has left the buffer
        if self.host is None or self.host.numel() < at:
            self.host = torch.empty(max(at, 4), dtype=torch.uint8, pin_memory=self.pin)
        buf = self.host.numpy()
        for s_off, b_off, f in place.values():
            buf[s_off:s_off + len(f.stream)] = np.frombuffer(f.stream, dtype=np.uint8)
            if b_off >= 0:
                buf[b_off:b_off + len(f.bitmap)] = np.frombuffer(f.bitmap, dtype=np.uint8)
        pitch = (ni * nj + 3) // 4 * 4
        current = torch.cuda.current_stream(self.device)
        self.copy_stream.wait_stream(current)
        with torch.cuda.stream(self.copy_stream):
            dev = self.host[:max(at, 4)].to(self.device, non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record(self.copy_stream)
        current.wait_stream(self.copy_stream)      # the unpack launches run after the transfer
        dev.record_stream(current)
        flat, self.last_status = decode_placed(dev, chosen, [place[path, id(m)][:2] for path, m, _ in chosen], pitch, self.check)
        # no copy: where Nj * Ni is no multiple of 4 the planes keep their pitch (dense planes, which load_native_batch takes as they are)
        planes = flat.as_strided((F, B, T, nj, ni), (B * T * pitch, T * pitch, pitch, ni, 1))
        return planes, lat.copy(), lon.copy()


def convert_titan_grib_to_npy(dataset, device=None, batch: int = 8) -> List[Path]:
    """``convert_samples_grib2_numpy`` of the reference's ``prepare --convert-grib2npy`` (datasets/titan/titan_cli.py:17-44) on the
    device: for every validity date of every sample of ``dataset`` -- the samples whose GRIB files exist -- and every parameter whose
    ``.npy`` is not there yet, the float32 sub-domain plane, un-standardised, goes to ``titan_plane_path``.  The planes of up to
    ``batch`` dates come from one pass of ``datasets.GribRoutes``: the window kernel with mean 0 and std 1 for parameters already on
    the target grid, unpack + regrid for the others.  A date whose GRIB cannot be read (missing, malformed, a message not found or on another grid) prints the reference's
    warning and is skipped; any other error, a device error among them, propagates.
    ``file_format`` and ``standardize`` are put back afterwards.  -> the files written, in order."""
    from . import datasets as D

    s, acc = dataset.settings, dataset.accessor
    if device is None:
        if not torch.cuda.is_available():
            raise ValueError("convert_titan_grib_to_npy: a CUDA device is needed: the decode and the regrid have no host path")
        device = torch.device("cuda", torch.cuda.current_device())
    keep = (s.file_format, s.standardize)
    written: List[Path] = []
    # what "cannot be read" means: a file or message that is missing or malformed (GribError is a ValueError; a complex-packed stream
    # that contradicts its header raises it after the decode).  An error of the device or of this code is not among them and ends the run.
    unreadable = (D.PlaneReadError, OSError, KeyError, ValueError)

    def target(p, date):
        return titan_plane_path(acc.get_dataset_path(s.dataset_name, dataset.grid), p.name, p.level, p.level_type, date)

    def convert(params, dates):
        planes = routes.planes(params, dates, device).cpu().numpy()
        for b, date in enumerate(dates):
            for f, p in enumerate(params):
                path = target(p, date)
                path.parent.mkdir(parents=True, exist_ok=True)
                np.save(path, np.ascontiguousarray(planes[b, :, :, f], dtype=np.float32))
                written.append(path)

    try:
        s.file_format, s.standardize = "grib", False      # the GRIB files define the valid samples
        dataset.__dict__.pop("sample_list", None)
        routes = D.GribRoutes(dataset)
        todo: "OrderedDict[dt.datetime, tuple]" = OrderedDict()
        for sample in dataset.sample_list:
            for date in sample.timestamps.validity_times:
                if date not in todo:          # the parameters it misses, as indices (a WeatherParam is not hashable)
                    todo[date] = tuple(i for i, p in enumerate(sample.params) if not target(p, date).exists())
        for missing in dict.fromkeys(todo.values()):      # dates that miss the same parameters go together
            params = [dataset.params[i] for i in missing]
            dates = [d for d, m in todo.items() if m == missing]
            for k in range(0, len(dates) if params else 0, max(int(batch), 1)):
                chunk = dates[k:k + max(int(batch), 1)]
                try:
                    convert(list(params), chunk)
                except unreadable:
                    for date in chunk:                    # one of them cannot be read: date by date, as the reference goes
                        try:
                            if not all(target(p, date).exists() for p in params):
                                convert([p for p in params if not target(p, date).exists()], [date])
                        except unreadable as e:
                            p = getattr(e, "param", params[0])
                            print(e)
                            print(f"WARNING: Could not load grib {acc.parameter_namer(p)} {p.level} {date}. Skipping.")
    finally:
        s.file_format, s.standardize = keep
        dataset.__dict__.pop("sample_list", None)
    return written


def load_titan_grib_batch(dataset_path, params: List[Tuple[str, str, dict, str]], dates: List[List[dt.datetime]], stats: Stats,
                          num_input_steps: int, forcing, plans: Dict[str, object], reader: Optional[GribPlaneReader] = None, device=None,
                          standardize: bool = True):
    """``load_titan_batch`` for Titan's GRIB layout (``file_format="grib"``, the reference's default): one ``GribPlaneReader`` call per
    native grid, then ``datapipe.load_native_batch`` (fit_to_grid, the latitude flip, the sub-domain, the standardisation and the
    pack in one launch).  params: (feature name, grib_name, fid, native grid name), ``fid`` the numeric keys of the message
    (``outputs.grib_fid``); dates[b][t]: validity times of sample b; plans: native grid name -> ``regrid.RegridPlan``.  Returns the
    ItemBatch of ``load_titan_batch`` on the reader's device.  There is no host path: the regrid runs on the device only."""
    from . import datapipe

    if not params:
        raise ValueError("load_titan_grib_batch: no parameters")
    if not dates or not dates[0] or any(len(d) != len(dates[0]) for d in dates):
        raise ValueError("load_titan_grib_batch: dates[b][t] must have the same, non-zero number of steps for every sample")
    names = [p[0] for p in params]
    if len(set(names)) != len(names):
        raise ValueError(f"load_titan_grib_batch: feature names {sorted(n for n in set(names) if names.count(n) > 1)} appear twice")
    missing = sorted({p[3] for p in params} - set(plans))
    if missing:
        raise ValueError(f"load_titan_grib_batch: no plan for the native grids {missing}")
    if not 0 < num_input_steps <= len(dates[0]):
        raise ValueError(f"load_titan_grib_batch: {num_input_steps} input steps of {len(dates[0])} dates")
    if reader is None:
        reader = GribPlaneReader(device=device)
    if not reader.cuda:
        raise ValueError("load_titan_grib_batch: a CUDA device (or a reader on one) is needed: the regrid has no host path")
    groups = []
    for grid in dict.fromkeys(p[3] for p in params):          # the grids in the order of their first parameter
        mine = [p for p in params if p[3] == grid]
        selections = [[[(titan_grib_path(dataset_path, grib_name, d), fid) for d in sample] for sample in dates] for (_, grib_name, fid, _) in mine]
        planes, _, _ = reader.read(selections)
        groups.append((planes, [p[0] for p in mine], plans[grid]))
    return datapipe.load_native_batch(groups, names, forcing, stats, num_input_steps, standardize)
