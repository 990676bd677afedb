"""
Input pipeline step right before the hot path: the reference standardises every parameter on the
CPU with numpy (``Sample.get_param_tensor``, datasets/base.py:431-453), concatenates the parameters along the feature
axis (``Sample.load`` :455-527) and stacks samples (``collate_fn`` :173-195).  Here the RAW parameter planes go to the
device as they come from disk (one plane per parameter) and ONE kernel standardises and packs them into the
features-last batch layout the rollout consumes.
"""

from datetime import datetime, timedelta
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import forcings, ops, regrid
from .base import ItemBatch
from .namedtensor import NamedTensor

DIMS = ["batch", "timestep", "lat", "lon", "features"]


def standardize_and_collate(raw: torch.Tensor, feature_names: Sequence[str], stats, standardize: bool = True) -> NamedTensor:
    """raw: (F, B, T, H, W) device tensor of un-normalised parameter planes -> NamedTensor (B,T,H,W,F) fp32."""
    F = raw.shape[0]
    if standardize:
        mean = stats.to_list("mean", list(feature_names)).to(raw.device)
        std = stats.to_list("std", list(feature_names)).to(raw.device)
    else:
        mean, std = torch.zeros(F, device=raw.device), torch.ones(F, device=raw.device)
    return NamedTensor(ops.pack_standardize(raw, mean, std), DIMS.copy(), list(feature_names))


def load_batch(raw_io: torch.Tensor, io_names: List[str], forcing: NamedTensor, stats, num_input_steps: int,
               standardize: bool = True) -> ItemBatch:
    """Device-side ``Sample.load`` + ``collate_fn`` for input_output parameters: the first ``num_input_steps`` time
    steps are the inputs, the rest the targets (base.py:493-505)."""
    full = standardize_and_collate(raw_io, io_names, stats, standardize)
    t = full.tensor
    inputs = NamedTensor(t[:, :num_input_steps], DIMS.copy(), list(io_names))
    outputs = NamedTensor(t[:, num_input_steps:], DIMS.copy(), list(io_names))
    return ItemBatch(inputs=inputs, forcing=forcing, outputs=outputs)


class PlaneTransform(NamedTuple):
    """What an accessor does to a plane between the file and the standardisation: ``np.where(arr < floor, floor, arr)``, ``/ div``,
    ``* mul`` and ``arr[::-1]``.  The default changes nothing."""
    floor: Optional[float] = None
    div: float = 1.0
    mul: float = 1.0
    flip: bool = False


# datasets/rainfall.py:150-155: 0 outside of the radar field, mm 10^-2 in 5 minutes -> mm/h, latitude inverted
RAINFALL_TRANSFORM = PlaneTransform(floor=0.0, div=100.0, mul=12.0, flip=True)


def _transform_list(transforms, names) -> List[PlaneTransform]:
    if transforms is None:
        return [PlaneTransform()] * len(names)
    if isinstance(transforms, PlaneTransform):
        return [transforms] * len(names)
    if isinstance(transforms, dict):
        return [transforms.get(n) or PlaneTransform() for n in names]
    transforms = [t or PlaneTransform() for t in transforms]
    if len(transforms) != len(names):
        raise ValueError(f"{len(transforms)} transforms for {len(names)} features")
    return transforms


def pack_typed_host(planes, transforms, mean, std) -> torch.Tensor:
    """The host statement of ``p4c_pack_convert`` (include/py4cast_hip.h), numpy float32 step by step: what a loader on the CPU
    device returns and what the kernel is tested against.  planes: per feature a (B, T, H, W) array in its file dtype."""
    f4, cols = np.float32, []
    with np.errstate(all="ignore"):
        for x, tr, m, s in zip(planes, transforms, mean, std):
            v = np.asarray(x).astype(f4)
            if tr.floor is not None:
                v = np.where(v < f4(tr.floor), f4(tr.floor), v)
            if f4(tr.div) != f4(1):
                v = v / f4(tr.div)
            if f4(tr.mul) != f4(1):
                v = v * f4(tr.mul)
            if tr.flip:
                v = v[..., ::-1, :]
            cols.append((v - f4(m)) / f4(s))
    return torch.from_numpy(np.ascontiguousarray(np.stack(cols, axis=-1), dtype=f4))


def pack_typed(raw, names: Sequence[str], transforms, stats, standardize: bool = True, host: bool = False) -> torch.Tensor:
    """Planes in their file dtype -> (B, T, H, W, F) fp32 standardised features-last.  raw: one (F, B, T, H, W) tensor or one
    tensor per feature ((B, T, H, W) or (1, B, T, H, W)), all of one dtype on one device.  Planes that are not on a CUDA device
    are refused like every other op of the package (no CPU fallback) unless ``host=True`` asks for the host statement
    (``pack_typed_host``: numpy arrays and CPU tensors).  On a CUDA device this is one launch:
    ``p4c_pack_standardize`` for untransformed fp32 planes in one tensor, ``p4c_pack_convert`` for everything else."""
    names = list(names)
    trs = _transform_list(transforms, names)
    if standardize:
        mean, std = stats.to_list("mean", names).tolist(), stats.to_list("std", names).tolist()
    else:
        mean, std = [0.0] * len(names), [1.0] * len(names)

    def as_numpy(t):
        return t if isinstance(t, np.ndarray) else (t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.uint16 else t.numpy())

    single = isinstance(raw, (torch.Tensor, np.ndarray))
    sources = [raw] if single else [r if r.ndim == 5 else r[None] for r in raw]
    where = [(si, k) for si, s in enumerate(sources) for k in range(s.shape[0])]
    if len(where) != len(names) or any(s.ndim != 5 for s in sources):
        raise ValueError(f"pack_typed: {len(where)} planes of shapes {[tuple(s.shape) for s in sources]} for {len(names)} names")
    B, T, H, W = sources[0].shape[1:]
    if isinstance(sources[0], np.ndarray) or not sources[0].is_cuda:
        if not host:
            raise ops.L.P4CError("pack_typed: the planes are not on a CUDA device and the kernels run on the GPU only (no CPU fallback); "
                                 "host=True asks for the numpy statement of the same arithmetic")
        return pack_typed_host([as_numpy(sources[si])[k] for si, k in where], trs, mean, std)
    plain = all(t == PlaneTransform() for t in trs)
    if plain and len(sources) == 1 and sources[0].dtype == torch.float32 and sources[0].is_contiguous():
        dev = sources[0].device
        return ops.pack_standardize(sources[0], torch.tensor(mean, device=dev), torch.tensor(std, device=dev))
    feats = [(si, k, tr.floor, tr.div, tr.mul, tr.flip, mean[c], std[c], c) for c, ((si, k), tr) in enumerate(zip(where, trs))]
    return ops.pack_convert(sources, feats, B, T, H, W)


def load_typed_batch(raw, io_names: List[str], transforms, forcing: NamedTensor, stats, num_input_steps: int,
                     standardize: bool = True, host: bool = False) -> ItemBatch:
    """``load_batch`` for planes that are still in their file's number format (u8, i16, u16, i32, f16, f32, f64) and still need the
    accessor's transform (``PlaneTransform``; the rainfall accessor's is ``RAINFALL_TRANSFORM``): conversion, transform,
    standardisation and pack are ONE pass of ``p4c_pack_convert``, no host ``astype``.  raw, transforms, host: as ``pack_typed``
    takes them.  -> the ItemBatch of ``load_batch``."""
    io_names = list(io_names)
    full = pack_typed(raw, io_names, transforms, stats, standardize, host)
    inputs = NamedTensor(full[:, :num_input_steps], DIMS.copy(), io_names)
    outputs = NamedTensor(full[:, num_input_steps:], DIMS.copy(), list(io_names))
    return ItemBatch(inputs=inputs, forcing=forcing, outputs=outputs)


def load_native_batch(groups, io_names: List[str], forcing: NamedTensor, stats, num_input_steps: int,
                      standardize: bool = True) -> ItemBatch:
    """``load_batch`` for planes still on their NATIVE grids: the reference's ``fit_to_grid`` (datasets/titan/__init__.py:184-208),
    the latitude flip of ``load_data_for_date`` and the sub-domain of titan_cli.py:36, standardised and packed by ONE
    ``p4c_regrid_pack`` launch for the whole batch (after one ``p4c_regrid_blur`` launch per group whose plan has a Gaussian);
    no full-grid plane exists.  ``py4cast_amd/regrid.py`` has the definition.

    groups: a list of (raw (Fg, B, T, Hs, Ws) device tensor, its Fg names, RegridPlan), all plans on one sub-domain of one
    full grid; io_names: the output feature order, every name from exactly one group.  -> the ItemBatch of ``load_batch``."""
    io_names = list(io_names)
    if not groups:
        raise ValueError("load_native_batch: no groups")
    if not 1 <= len(io_names) <= ops.REGRID_MAX_FEATURES:
        raise ValueError(f"load_native_batch: {len(io_names)} features: 1 .. at most {ops.REGRID_MAX_FEATURES} per call (LDS tile)")
    first = groups[0][2]
    where = {}
    for gi, (raw, names, plan) in enumerate(groups):
        names = list(names)
        if raw.dim() != 5 or raw.shape[0] != len(names) or tuple(raw.shape[3:]) != plan.src_shape:
            raise ValueError(f"load_native_batch: group {gi}: raw {tuple(raw.shape)} is not (Fg, B, T, Hs, Ws) with Fg = {len(names)} "
                             f"names and (Hs, Ws) = {plan.src_shape}")
        if tuple(raw.shape[1:3]) != tuple(groups[0][0].shape[1:3]):
            raise ValueError(f"load_native_batch: group {gi} has batch x steps {tuple(raw.shape[1:3])}, group 0 {tuple(groups[0][0].shape[1:3])}")
        if (plan.full_size, plan.subdomain) != (first.full_size, first.subdomain):
            raise ValueError(f"load_native_batch: group {gi} is on sub-domain {plan.subdomain} of {plan.full_size}, group 0 on "
                             f"{first.subdomain} of {first.full_size}: one launch writes one sub-domain")
        for k, name in enumerate(names):
            if name in where:
                raise ValueError(f"load_native_batch: feature {name!r} is in groups {where[name][0]} and {gi}")
            where[name] = (gi, k)
    if sorted(where) != sorted(io_names):
        raise ValueError(f"load_native_batch: io_names and the groups' names differ: {sorted(set(where) ^ set(io_names))}")
    ops.L.require_cuda(*(g[0] for g in groups))
    dev = groups[0][0].device
    B, T = groups[0][0].shape[1:3]
    if standardize:
        mean, std = stats.to_list("mean", io_names).tolist(), stats.to_list("std", io_names).tolist()
    else:
        mean, std = [0.0] * len(io_names), [1.0] * len(io_names)
    keys, plans, sources, windows, src_bytes = {}, [], [], [], 0
    for raw, names, plan in groups:
        if plan.key not in keys:
            keys[plan.key] = len(plans)
            plans.append(plan)
        raw = raw.float()
        src, window = regrid.blurred(raw if ops.planes_dense(raw) else raw.contiguous(), plan)     # planes at a pitch stay where they are
        sources.append(src)
        windows.append(window)
        src_bytes += regrid.source_bytes(plan, len(names) * B * T)
    feats = []
    for channel, name in enumerate(io_names):
        gi, k = where[name]
        feats.append((gi, k, windows[gi][0], windows[gi][2], keys[groups[gi][2].key], mean[channel], std[channel], channel))
    feats.sort(key=lambda f: (f[4], f[0], f[1]))      # features of one tap table side by side: their table reads hit
    full = ops.regrid_pack(sources, feats, regrid.device_taps(plans, dev), [p.n for p in plans], B, T, *first.out_shape,
                           src_bytes=src_bytes)
    inputs = NamedTensor(full[:, :num_input_steps], DIMS.copy(), io_names)
    outputs = NamedTensor(full[:, num_input_steps:], DIMS.copy(), list(io_names))
    return ItemBatch(inputs=inputs, forcing=forcing, outputs=outputs)


class WindowTable(NamedTuple):
    """What ``load_window_batch`` launches with: ``fields`` (B, T, F) ``ops.GRIB_WFIELD`` records (mean 0, std 1: the batch call fills
    them in), the F feature ``names`` of its last axis and the sub-domain's ``shape`` (H, W)."""
    fields: np.ndarray
    names: tuple
    shape: tuple


def window_rows(plan) -> tuple:
    """(first, end) of the NORTH-FIRST native plane rows an identity ``plan`` reads: the rows ``grib2.window_slice`` has to ship"""
    if not plan.identity:
        raise ValueError("window_rows: the plan resizes; only a plane already on the target grid is read through a window")
    rows = plan.window[0] + plan.row_taps["i0"].astype(np.int64)
    return int(rows.min()), int(rows.max()) + 1


def window_qualifies(field, plan) -> bool:
    """a field ``p4c_grib_window_pack`` decodes: simple-packed, no bitmap, already on the target grid (an identity plan of its size)"""
    from . import grib2

    return bool(grib2.window_qualifies(field) and plan.identity and (field.nj, field.ni) == plan.src_shape)


def window_table(fields, places, names: Sequence[str], plan) -> WindowTable:
    """fields[f][b][t]: ``grib2.PackedField``s that ``window_qualifies``; places[f][b][t] = (slice_off, slice_len, bit0): where the
    field's slice (``grib2.window_slice`` over ``window_rows(plan)``) lies in the byte buffer and the bit of the stream it starts at;
    plan: the identity ``RegridPlan`` they share.  The plan's flip, window and sub-domain and each file's scanning direction are folded
    into ``row0`` / ``row_step`` / ``col0``."""
    F, B, T = len(fields), len(fields[0]), len(fields[0][0])
    if len(names) != F:
        raise ValueError(f"window_table: {len(names)} names for {F} features")
    H, W = plan.out_shape
    prow = plan.window[0] + plan.row_taps["i0"].astype(np.int64)       # north-first native row of every output row
    step = int(prow[1] - prow[0]) if H > 1 else 1
    if not plan.identity or (H > 1 and (abs(step) != 1 or not np.array_equal(np.diff(prow), np.full(H - 1, step)))):
        raise ValueError("window_table: the plan is no identity: its rows are not consecutive plane rows")
    col0 = int(plan.window[2] + plan.col_taps["i0"][0])
    table = np.zeros((B, T, F), dtype=ops.GRIB_WFIELD)
    table["bitmap_off"], table["std"] = -1, 1.0
    for fi in range(F):
        for b in range(B):
            for t in range(T):
                f = fields[fi][b][t]
                if not window_qualifies(f, plan):
                    raise ValueError(f"window_table: feature {names[fi]!r}, sample {b}, step {t}: not a simple-packed field without bitmap "
                                     f"on the plan's {plan.src_shape} grid")
                rec = table[b, t, fi]
                rec["slice_off"], rec["slice_len"], rec["bit0"] = places[fi][b][t]
                rec["ni"], rec["nbits"], rec["E"], rec["D"], rec["R"], rec["col0"] = f.ni, f.nbits, f.E, f.D, f.R, col0
                rec["row0"] = f.nj - 1 - int(prow[0]) if f.south_to_north else int(prow[0])
                rec["row_step"] = -step if f.south_to_north else step
    return WindowTable(table, tuple(names), (H, W))


def load_window_batch(bytes_dev: torch.Tensor, table: WindowTable, io_names: List[str], forcing: NamedTensor, stats,
                      num_input_steps: int, standardize: bool = True) -> ItemBatch:
    """``load_native_batch`` for fields that need no native plane at all: simple-packed, without bitmap, already on the target grid
    (``window_qualifies``).  The slices of their bit streams that hold the sub-domain's rows lie in ``bytes_dev``
    (``grib2.window_slice``), and ONE ``p4c_grib_window_pack`` launch decodes the window's values, standardises them and packs them
    features-last: the bits of ``ops.grib_unpack`` followed by ``load_native_batch`` with the identity plan.  table: ``window_table``'s;
    io_names: the output feature order, a permutation of the table's names.  -> the ItemBatch of ``load_batch``."""
    io_names = list(io_names)
    if sorted(io_names) != sorted(table.names) or len(set(io_names)) != len(io_names):
        raise ValueError(f"load_window_batch: io_names and the table's names differ: {sorted(set(table.names) ^ set(io_names))}")
    B, T, F = table.fields.shape
    if not 0 < num_input_steps <= T:
        raise ValueError(f"load_window_batch: {num_input_steps} input steps of {T}")
    order = [table.names.index(n) for n in io_names]
    fields = np.ascontiguousarray(table.fields[:, :, order])
    if standardize:
        fields["mean"] = np.asarray(stats.to_list("mean", io_names).tolist(), dtype=np.float32)
        fields["std"] = np.asarray(stats.to_list("std", io_names).tolist(), dtype=np.float32)
    else:
        fields["mean"], fields["std"] = 0.0, 1.0
    full = ops.grib_window_pack(bytes_dev, fields, B, T, *table.shape, F)
    inputs = NamedTensor(full[:, :num_input_steps], DIMS.copy(), io_names)
    outputs = NamedTensor(full[:, num_input_steps:], DIMS.copy(), list(io_names))
    return ItemBatch(inputs=inputs, forcing=forcing, outputs=outputs)


def build_forcing(raw: Optional[torch.Tensor], ext_names: Sequence[str], stats, dates: Sequence[datetime],
                  timedeltas: Sequence[timedelta], lat, lon, standardize: bool = True, device=None) -> NamedTensor:
    """Device-side forcing of ``Sample.load`` (base.py:455-527): the ``kind == "input"`` parameters standardised, then the five
    channels of ``generate_forcings`` (base.py:233-274) -- date values and top-of-atmosphere irradiance -- computed in the
    kernel from B run dates, T lead times and the grid's coordinates.

    raw: (Ff_ext, B, T, H, W) device tensor of un-normalised planes, or None (the dummy dataset: the five channels only);
    lat, lon: (H, W) in degrees.  -> NamedTensor (B, T, H, W, Ff_ext + 5) fp32, features ``ext_names + FORCING_NAMES`` (the
    concatenation order of base.py:509-515): what ``load_batch`` and ``diskio.load_titan_batch`` take as ``forcing``."""
    ext_names = list(ext_names)
    B, T = len(dates), len(timedeltas)
    lat_shape, lon_shape = tuple(getattr(lat, "shape", ())), tuple(getattr(lon, "shape", ()))
    if len(lat_shape) != 2 or lon_shape != lat_shape:
        raise ValueError(f"build_forcing: lat {lat_shape} and lon {lon_shape} must be the same (H, W)")
    H, W = lat_shape
    if B == 0 or T == 0:
        raise ValueError("build_forcing: needs at least one date and one lead time")
    if raw is None:
        if ext_names:
            raise ValueError(f"build_forcing: {len(ext_names)} external feature names and no raw planes")
    else:
        if raw.dim() != 5 or raw.shape[0] != len(ext_names):
            raise ValueError(f"build_forcing: raw {tuple(raw.shape)} is not (Ff_ext, B, T, H, W) with Ff_ext = {len(ext_names)} names")
        if raw.shape[1] != B or raw.shape[2] != T:
            raise ValueError(f"build_forcing: {B} dates x {T} lead times for raw planes of batch {raw.shape[1]} x {raw.shape[2]} steps")
        if tuple(raw.shape[3:]) != (H, W):
            raise ValueError(f"build_forcing: lat / lon {lat_shape} do not match the planes' grid {tuple(raw.shape[3:])}")
        if device is None:
            device = raw.device
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    mean = std = None
    if raw is not None and raw.shape[0] > 0:
        if standardize:
            mean, std = stats.to_list("mean", ext_names).to(device), stats.to_list("std", ext_names).to(device)
        else:
            mean, std = torch.zeros(len(ext_names), device=device), torch.ones(len(ext_names), device=device)
    table = forcings.time_table(dates, timedeltas).to(device)
    planes = forcings.grid_tables(lat, lon, device)
    out = ops.build_forcing(raw, mean, std, table, planes, B, T, H, W)
    return NamedTensor(out, DIMS.copy(), ext_names + forcings.FORCING_NAMES)
