"""
Native-grid planes onto the training sub-domain: the host side of ``p4c_regrid_pack`` / ``p4c_regrid_blur``.

Titan's parameters do not start on one grid (datasets/titan/metadata.yaml: ARPEGE on PA_01D, most AROME fields on
PAAROME_1S40, the target PAAROME_1S100 or PAAROME_1S40).  The reference bridges that on the CPU, one plane at a time:
``fit_to_grid`` (datasets/titan/__init__.py:184-208) crops ARPEGE planes to the AROME box and calls
``skimage.transform.resize`` to the target grid's FULL size (``anti_aliasing`` only towards PAAROME_1S40),
``load_data_for_date`` inverts the latitude axis and titan_cli.py:36 cuts the sub-domain.  Here a ``RegridPlan`` holds
that chain as tables and the kernel computes the sub-domain's pixels only.

Definition.  For a 2-D float image and the defaults ``fit_to_grid`` uses (order 1, mode "reflect", clip), resize of
skimage >= 0.19 is, in ``scipy.ndimage``::

    factors = in_shape / out_shape
    if anti_aliasing:
        img = ndi.gaussian_filter(img, sigma=max(0, (factors - 1) / 2), mode="mirror")
    out = ndi.zoom(img, 1 / factors, order=1, mode="mirror", grid_mode=True)

THIS ``scipy.ndimage`` form is the stated definition (tests/golden/make_golden_regrid.py generates the expected values with
it).  skimage is not a dependency of this project and parity with skimage itself is UNPINNED: no test here has run it.

Per axis, source length n (after the window crop) and full target length N:
  * output index o has the source coordinate x = ((2o + 1) n - N) / (2N), formed here as an exact integer fraction;
  * mirror: x < 0 -> -x, x > n - 1 -> 2(n - 1) - x (the edge pixel is not repeated: period 2(n - 1));
  * taps i0 = floor(x), i1 = min(i0 + 1, n - 1), f = x - i0 (rounded to fp32 once);
  * blur: sigma = max(0, (n / N - 1) / 2), radius int(4 sigma + 0.5), weights exp(-k^2 / 2 sigma^2) normalised to sum 1,
    mirror indexing modulo the period at the edges of the WINDOWED array.
Chain order: window crop -> blur -> resize -> latitude flip -> sub-domain -> fp32 -> (v - mean) / std -> features-last pack.
A plane already on the target grid (n == N on both axes) is an identity: x = o, f = 0, flip and sub-domain only.

This module needs no GPU to import or to build a plan; ``fit_to_grid`` and ``datapipe.load_native_batch`` launch.
"""

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

MAX_RADIUS = 64      # p4c_regrid_blur's limit
TRUNCATE = 4.0       # scipy.ndimage.gaussian_filter's default


def titan_window(lats, lons, extent) -> Tuple[int, int, int, int]:
    """The crop of ``fit_to_grid`` (datasets/titan/__init__.py:200-204) as a window (r0, r1, c0, c1), ends exclusive:
    the rows with extent[1] <= lat <= extent[0] and the columns with extent[2] <= lon <= extent[3], for 1-D ``lats`` /
    ``lons`` and ``extent`` = (north, south, west, east) as the reference's grids store it.  The boolean masks of the
    reference select a block only when they are contiguous: anything else raises."""
    lats, lons = np.asarray(lats), np.asarray(lons)
    if lats.ndim != 1 or lons.ndim != 1:
        raise ValueError(f"titan_window: lats {lats.shape} and lons {lons.shape} must be 1-D")
    out = []
    for what, mask in (("latitudes", (lats >= extent[1]) & (lats <= extent[0])), ("longitudes", (lons >= extent[2]) & (lons <= extent[3]))):
        idx = np.flatnonzero(mask)
        if idx.size == 0:
            raise ValueError(f"titan_window: no {what} inside the extent {tuple(extent)}")
        if idx[-1] - idx[0] + 1 != idx.size:
            raise ValueError(f"titan_window: the {what} inside the extent {tuple(extent)} are not contiguous")
        out += [int(idx[0]), int(idx[-1]) + 1]
    return tuple(out)


def _axis_taps(n: int, N: int, outputs: np.ndarray) -> np.ndarray:
    """tap entries (ops.REGRID_TAP) of the resized-axis indices ``outputs``: integer arithmetic up to the one division"""
    o = outputs.astype(np.int64)
    den = 2 * N
    num = (2 * o + 1) * n - N
    num = np.where(num < 0, -num, num)
    top = (n - 1) * den
    num = np.where(num > top, 2 * top - num, num)
    i0 = num // den
    taps = np.zeros(len(o), dtype=ops.REGRID_TAP)
    taps["i0"], taps["i1"] = i0, np.minimum(i0 + 1, n - 1)
    taps["f"] = ((num - i0 * den).astype(np.float64) / den).astype(np.float32)
    return taps


def _axis_blur(n: int, N: int, anti_aliasing: bool):
    sigma = max(0.0, (n / N - 1) / 2) if anti_aliasing else 0.0
    radius = int(TRUNCATE * sigma + 0.5)
    if radius > MAX_RADIUS:
        raise ValueError(f"RegridPlan: {n} -> {N} points needs a Gaussian of radius {radius}: at most {MAX_RADIUS}")
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 * k * k / (sigma * sigma)) if radius > 0 else np.ones(1)
    pos = np.arange(-radius, n + radius) % (2 * (n - 1))
    return sigma, radius, w / w.sum(), np.where(pos > n - 1, 2 * (n - 1) - pos, pos).astype(np.int32)


class RegridPlan:
    """One geometry of the chain: planes of ``src_shape``, cropped to ``window`` (r0, r1, c0, c1; None: the whole plane),
    resized to ``full_size``, flipped along the latitude axis (``flip_lat``), cut to ``subdomain`` (a, b, c, d) = rows a:b,
    columns c:d of the flipped full-size plane (None: all of it).

    n, N, sigma, radius, weights: per axis (rows, columns).  row_taps / col_taps: ops.REGRID_TAP arrays, one entry per row /
    column of the sub-domain, flip and sub-domain origin folded in.  row_index / col_index: the blur's mirrored source
    indices.  key: plans with an equal key have equal tables whatever their window origin or plane size."""

    def __init__(self, src_shape: Sequence[int], full_size: Sequence[int], window: Optional[Sequence[int]] = None,
                 subdomain: Optional[Sequence[int]] = None, anti_aliasing: bool = False, flip_lat: bool = True):
        self.src_shape = tuple(int(s) for s in src_shape)
        self.full_size = tuple(int(s) for s in full_size)
        if len(self.src_shape) != 2 or len(self.full_size) != 2 or min(self.full_size) < 1:
            raise ValueError(f"RegridPlan: src_shape {src_shape} and full_size {full_size} must be (rows, columns)")
        Hs, Ws = self.src_shape
        self.window = (0, Hs, 0, Ws) if window is None else tuple(int(v) for v in window)
        r0, r1, c0, c1 = self.window
        if not (0 <= r0 < r1 <= Hs and 0 <= c0 < c1 <= Ws):
            raise ValueError(f"RegridPlan: window {self.window} does not lie inside planes of {self.src_shape}")
        self.n, self.N = (r1 - r0, c1 - c0), self.full_size
        if min(self.n) < 2:
            raise ValueError(f"RegridPlan: a windowed source of {self.n}: each axis needs at least 2 points (mirror period 2(n - 1))")
        self.subdomain = (0, self.N[0], 0, self.N[1]) if subdomain is None else tuple(int(v) for v in subdomain)
        a, b, c, d = self.subdomain
        if not (0 <= a < b <= self.N[0] and 0 <= c < d <= self.N[1]):
            raise ValueError(f"RegridPlan: sub-domain {self.subdomain} does not lie inside the full grid {self.N}")
        self.out_shape = (b - a, d - c)
        self.anti_aliasing, self.flip_lat = bool(anti_aliasing), bool(flip_lat)
        self.identity = self.n == self.N
        blur = [_axis_blur(n, N, self.anti_aliasing) for n, N in zip(self.n, self.N)]
        self.sigma, self.radius = tuple(x[0] for x in blur), tuple(x[1] for x in blur)
        self.weights = tuple(x[2] for x in blur)
        self.row_index, self.col_index = blur[0][3], blur[1][3]
        self.needs_blur = max(self.radius) > 0
        rows = np.arange(a, b)
        self.row_taps = _axis_taps(self.n[0], self.N[0], self.N[0] - 1 - rows if self.flip_lat else rows)
        self.col_taps = _axis_taps(self.n[1], self.N[1], np.arange(c, d))
        self.key = (self.n, self.N, self.subdomain, self.flip_lat)
        self.blur_key = (self.n, self.N) if self.needs_blur else None

    @property
    def footprint(self) -> Tuple[int, int]:
        """(rows, columns) of the windowed source the sub-domain's taps span: the algorithmic read of one plane"""
        rt, ct = self.row_taps, self.col_taps
        return int(rt["i1"].max() - rt["i0"].min() + 1), int(ct["i1"].max() - ct["i0"].min() + 1)


# device copies of the tables, shared by plans with equal geometry (a training run holds two or three)
_DEVICE_TABLES = {}


def _cached(key, device, make):
    key = (key, str(device))
    if key not in _DEVICE_TABLES:
        if len(_DEVICE_TABLES) >= 64:
            _DEVICE_TABLES.clear()
        _DEVICE_TABLES[key] = make()
    return _DEVICE_TABLES[key]


def device_taps(plans: Sequence[RegridPlan], device) -> torch.Tensor:
    """(tables, H_sub + W_sub, 4) int32 on ``device``: per plan its row entries, then its column entries (p4c_regrid_tap)"""
    def make():
        host = np.stack([np.concatenate([p.row_taps, p.col_taps]) for p in plans])
        return torch.from_numpy(host.view(np.int32).reshape(len(plans), -1, 4)).to(device)

    return _cached(("taps",) + tuple(p.key for p in plans), device, make)


def device_blur_tables(plan: RegridPlan, device):
    """(row_index, col_index, row_w, col_w) of ``p4c_regrid_blur`` on ``device``; the weights rounded to fp32 once"""
    def make():
        return (torch.from_numpy(plan.row_index).to(device), torch.from_numpy(plan.col_index).to(device),
                torch.from_numpy(plan.weights[0].astype(np.float32)).to(device), torch.from_numpy(plan.weights[1].astype(np.float32)).to(device))

    return _cached(("blur", plan.blur_key), device, make)


def blurred(raw: torch.Tensor, plan: RegridPlan):
    """(source, window) the resize reads: ``raw`` (..., Hs, Ws) and the plan's window, or -- one ``p4c_regrid_blur`` launch,
    only when some axis has a radius > 0 -- the blurred window as a dense scratch tensor (..., n_rows, n_cols) and its whole
    extent"""
    if not plan.needs_blur:
        return raw, plan.window
    ri, ci, rw, cw = device_blur_tables(plan, raw.device)
    return ops.regrid_blur(raw, plan.window, ri, ci, rw, cw), (0, plan.n[0], 0, plan.n[1])


def source_bytes(plan: RegridPlan, planes: int) -> int:
    """algorithmic bytes the pack kernel reads from ``planes`` source planes of this geometry"""
    fr, fc = plan.footprint
    return 4 * fr * fc * planes


def fit_to_grid(planes, plan: RegridPlan, device=None) -> torch.Tensor:
    """``fit_to_grid`` + latitude flip + sub-domain of the reference for planes (..., Hs, Ws), numpy or tensor ->
    (..., H_sub, W_sub) fp32 on the device: the un-standardised product, what ``prepare`` would save.  One
    ``p4c_regrid_pack`` launch with mean 0 and std 1 (so (v - 0) / 1 = v exactly), every plane one single-feature image of it."""
    t = torch.from_numpy(np.ascontiguousarray(planes)) if isinstance(planes, np.ndarray) else planes
    if t.dim() < 2 or tuple(t.shape[-2:]) != plan.src_shape:
        raise ValueError(f"fit_to_grid: planes {tuple(t.shape)} are not (..., {plan.src_shape[0]}, {plan.src_shape[1]})")
    if device is not None:
        t = t.to(device)
    ops.L.require_cuda(t)
    lead = tuple(t.shape[:-2])
    raw = t.float().contiguous().reshape(1, -1, 1, *plan.src_shape)
    P = raw.shape[1]
    src, window = blurred(raw, plan)
    out = ops.regrid_pack([src], [(0, 0, window[0], window[2], 0, 0.0, 1.0, 0)], device_taps([plan], raw.device), [plan.n], P, 1,
                          *plan.out_shape, src_bytes=source_bytes(plan, P))
    return out.reshape(*lead, *plan.out_shape)
