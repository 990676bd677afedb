"""
torch.autograd wrappers around the rollout / loss entry points of ``libpy4cast_hip.so``.

These are thin: they validate layouts, pass raw device pointers + strides + the current
HIP stream through the C ABI and wire the matching backward entry point.  They allocate
outputs with the PyTorch caching allocator (the library owns no memory).
"""

import ctypes
import functools
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L

_KINDS = {"mse": L.LOSS_MSE, "MSELoss": L.LOSS_MSE, "l1": L.LOSS_L1, "L1Loss": L.LOSS_L1}


def loss_kind_code(kind) -> int:
    try:
        return _KINDS[kind]
    except KeyError:
        raise L.P4CError(f"unsupported torch loss {kind!r}: the HIP losses implement MSELoss and L1Loss") from None


def _rows(t: torch.Tensor, lead: int) -> Tuple[torch.Tensor, list]:
    """
    View ``t`` (lead dims..., *spatial, F) for the kernels: the trailing (*spatial, F) block must
    be dense; leading dims may carry arbitrary strides.  Returns (tensor, leading strides).
    """
    inner = 1
    ok = True
    for d in range(t.dim() - 1, lead - 1, -1):
        if t.size(d) != 1 and t.stride(d) != inner:
            ok = False
            break
        inner *= t.size(d)
    if not ok:
        t = t.contiguous()
    return t, [t.stride(d) if t.size(d) != 1 else 0 for d in range(lead)]


def _numel_spatial(t: torch.Tensor, lead: int) -> int:
    n = 1
    for d in range(lead, t.dim() - 1):
        n *= t.size(d)
    return n


def pad_channels(c: int, multiple: int = 16) -> int:
    return (c + multiple - 1) // multiple * multiple


# ------------------------------------------------------------------------------ K1
class _BuildX(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prev_states, statics, forcing_i, mask_on_nan, downscaling_only, c_pad, out_dtype, blocks=None):
        L.require_cuda(prev_states, statics, forcing_i)
        B, T_in = prev_states.shape[0], prev_states.shape[1]
        F, Fs, Ff = prev_states.shape[-1], statics.shape[-1], forcing_i.shape[-1]
        N = _numel_spatial(forcing_i, 1)
        prev, (pbs, pts) = _rows(prev_states.float(), 2)
        st, (sbs,) = _rows(statics.float(), 1)
        fo, (fbs,) = _rows(forcing_i.float(), 1)
        c_in = (0 if downscaling_only else T_in * F) + Fs + Ff + int(mask_on_nan)
        c_pad = c_in if c_pad is None else c_pad
        x = torch.empty(forcing_i.shape[:-1] + (c_pad,), dtype=out_dtype, device=forcing_i.device)
        args = (L.ptr(prev), pbs, pts, L.ptr(st), sbs, L.ptr(fo), fbs, L.ptr(x), L.dtype_code(out_dtype),
                c_pad, B, T_in, N, F, Fs, Ff, int(mask_on_nan), int(downscaling_only))
        if blocks is None:
            L.call("p4c_build_x", *args, L.stream(x.device))
        else:
            if forcing_i.dim() != 4:
                raise L.P4CError("build_x: the block mask needs the grid layout (B, H, W, features)")
            L.call("p4c_build_x_masked", *args, L.ptr(blocks.selected), forcing_i.shape[1], forcing_i.shape[2], blocks.block_h,
                   blocks.block_w, L.stream(x.device))
        ctx.meta = (B, T_in, N, F, c_pad, bool(downscaling_only), prev_states.shape, blocks, tuple(forcing_i.shape[1:3]))
        return x

    @staticmethod
    def backward(ctx, dx):
        B, T_in, N, F, c_pad, ds, shape, blocks, hw = ctx.meta
        if ds:
            return (torch.zeros(shape, dtype=torch.float32, device=dx.device),) + (None,) * 7
        dx = dx.contiguous()
        dprev = torch.empty(shape, dtype=torch.float32, device=dx.device)
        if blocks is None:
            L.call("p4c_build_x_bwd", L.ptr(dx), L.dtype_code(dx.dtype), c_pad, L.ptr(dprev), B, T_in, N, F, L.stream(dx.device))
        else:
            L.call("p4c_build_x_bwd_masked", L.ptr(dx), L.dtype_code(dx.dtype), c_pad, L.ptr(dprev), B, T_in, N, F,
                   L.ptr(blocks.selected), hw[0], hw[1], blocks.block_h, blocks.block_w, L.stream(dx.device))
        return (dprev,) + (None,) * 7


class BlockMask:
    """The draw of ``mask_tensor`` (lightning.py:769-785) as a table: ``selected`` (H*W,) uint8 on the device, 1 where the flat
    index was drawn; grid point (y, x) is cleared iff ``selected[(y // block_h) * W + x // block_w]``."""

    def __init__(self, selected: torch.Tensor, block_h: int, block_w: int):
        self.selected, self.block_h, self.block_w = selected, int(block_h), int(block_w)

    @staticmethod
    def draw(height: int, width: int, mask_ratio: float, device) -> "BlockMask":
        """Same arithmetic and the same torch CPU generator draw as the reference, so the same mask bit for bit."""
        num_blocks = int((1 - mask_ratio) * height * width)
        block_h = height // int(height**0.5)
        block_w = width // int(width**0.5)
        drawn = torch.randperm(height * width)[:num_blocks]
        selected = torch.zeros(height * width, dtype=torch.uint8)
        selected[drawn] = 1
        return BlockMask(selected.to(device), block_h, block_w)

    def dense(self, height: int, width: int) -> torch.Tensor:
        """(H, W) bool, True = kept (the reference's ``mask[0, :, :, 0]``); for observers and tests."""
        dev = self.selected.device
        by = torch.arange(height, device=dev) // self.block_h
        bx = torch.arange(width, device=dev) // self.block_w
        return self.selected[by[:, None] * width + bx[None, :]] == 0


def build_x(prev_states, statics, forcing_i, mask_on_nan=False, downscaling_only=False, c_pad=None, dtype=torch.float32,
            blocks: Optional[BlockMask] = None):
    """lightning.py:711-767.  prev_states (B,T_in,*S,F); statics (B,*S,Fs); forcing_i (B,*S,Ff) -> (B,*S,c_pad).
    ``blocks``: the masked-auto-encoder block mask (lightning.py:580-581, 769-785) applied in the same pass."""
    return _BuildX.apply(prev_states, statics, forcing_i, mask_on_nan, downscaling_only, c_pad, dtype, blocks)


# ------------------------------------------------------------------------------ K2
class _ARUpdate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prev, y, border_state, std, mean, border_mask, interior_mask, keep_prev, nan_to_num):
        L.require_cuda(y)
        B = y.shape[0]
        if prev is not None:
            F = prev.shape[-1]
        elif border_state is not None:
            F = border_state.shape[-1]
        else:
            F = std.numel() if std is not None else y.shape[-1]
        y_c = y.contiguous()
        y_cs = y_c.shape[-1]
        N = _numel_spatial(y_c, 1)
        pv, pbs = (None, 0)
        if prev is not None:
            pv, (pbs,) = _rows(prev.float(), 1)
        bsv, bbs = (None, 0)
        force = border_mask is not None
        if force:
            bsv, (bbs,) = _rows(border_state.float(), 1)
        new_state = torch.empty(y_c.shape[:-1] + (F,), dtype=torch.float32, device=y.device)
        L.call(
            "p4c_ar_update_fwd", L.ptr(pv), pbs, L.ptr(y_c), L.dtype_code(y_c.dtype), y_cs, L.ptr(bsv), bbs, L.ptr(std),
            L.ptr(mean), L.ptr(border_mask if force else None), L.ptr(interior_mask if force else None),
            L.ptr(new_state), N * F, B, N, F, float(keep_prev), int(nan_to_num), L.stream(y.device),
        )
        ctx.save_for_backward(std, interior_mask if force else None)
        ctx.meta = (B, N, F, y_cs, float(keep_prev), y.dtype, prev is not None, prev.shape if prev is not None else None)
        return new_state

    @staticmethod
    def backward(ctx, dnew):
        std, interior = ctx.saved_tensors
        B, N, F, y_cs, keep, ydt, has_prev, pshape = ctx.meta
        dnew, (dbs,) = _rows(dnew.float(), 1)
        dy = torch.empty(dnew.shape[:-1] + (y_cs,), dtype=ydt, device=dnew.device)
        dprev = torch.empty(pshape, dtype=torch.float32, device=dnew.device) if has_prev else None
        L.call(
            "p4c_ar_update_bwd", L.ptr(dnew), dbs, L.ptr(std), L.ptr(interior), L.ptr(dy), L.dtype_code(ydt), y_cs,
            L.ptr(dprev), N * F, B, N, F, keep, L.stream(dnew.device),
        )
        return dprev, dy, None, None, None, None, None, None, None


def ar_update(prev, y, border_state=None, std=None, mean=None, border_mask=None, interior_mask=None, keep_prev=1.0,
              nan_to_num=False):
    """lightning.py:599-633 in one pass.  masks are flat (N,) float tensors; returns fp32 (B,*S,F)."""
    return _ARUpdate.apply(prev, y, border_state, std, mean, border_mask, interior_mask, keep_prev, nan_to_num)


# ------------------------------------------------------------------------------ K3
class MaskSpec:
    """How the loss mask is provided (see p4c_mask_mode in include/py4cast_hip.h)."""

    def __init__(self, mode: int, tensor: Optional[torch.Tensor] = None):
        self.mode, self.tensor = mode, tensor

    @staticmethod
    def from_tensor(mask: Optional[torch.Tensor]) -> "MaskSpec":
        if mask is None:
            return MaskSpec(L.MASK_NONE)
        if mask.dtype == torch.bool:
            return MaskSpec(L.MASK_U8, mask.contiguous().view(torch.uint8))
        if mask.dtype == torch.uint8:
            return MaskSpec(L.MASK_U8, mask.contiguous())
        return MaskSpec(L.MASK_F32, mask.float().contiguous())


def masked_count(spec: MaskSpec, target: torch.Tensor) -> Optional[torch.Tensor]:
    """#grid points masked for every (b,t,f) -- the correction of losses.py:156,167.  None when mask==1."""
    if spec.mode == L.MASK_NONE:
        return None
    B, T, F = target.shape[0], target.shape[1], target.shape[-1]
    N = _numel_spatial(target, 2)
    count = torch.empty(1, dtype=torch.int32, device=target.device)
    if spec.mode == L.MASK_FROM_NAN:
        src, (bs, ts) = _rows(target, 2)
    else:
        src, bs, ts = spec.tensor, T * N * F, N * F
    L.call("p4c_mask_all_zero_count", L.ptr(src), spec.mode, bs, ts, B, T, N, F, L.ptr(count), L.stream(target.device))
    return count


def _workspace(B, T, N, F, device):
    nbytes = L.lib().p4c_loss_workspace_bytes(B, T, N, F)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


class _WeightedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, spec, weights, interior, num_interior, count, kind):
        L.require_cuda(pred, target)
        B, T, F = pred.shape[0], pred.shape[1], pred.shape[-1]
        N = _numel_spatial(pred, 2)
        p, (pbs, pts) = _rows(pred.float(), 2)
        g, (gbs, gts) = _rows(target.float(), 2)
        out = torch.empty(B, T, dtype=torch.float32, device=pred.device)
        ws = _workspace(B, T, N, F, pred.device)
        L.call(
            "p4c_weighted_loss_fwd", L.ptr(p), pbs, pts, L.ptr(g), gbs, gts, L.ptr(spec.tensor), spec.mode,
            L.ptr(weights), L.ptr(interior), float(num_interior), L.ptr(count), kind, L.ptr(out), L.ptr(ws), B, T, N, F,
            L.stream(pred.device),
        )
        ctx.save_for_backward(p, g, weights, interior, count, spec.tensor)
        ctx.meta = (spec.mode, float(num_interior), kind, pred.shape)
        return out

    @staticmethod
    def backward(ctx, gout):
        p, g, weights, interior, count, mtensor = ctx.saved_tensors
        mode, num_interior, kind, shape = ctx.meta
        B, T, F = shape[0], shape[1], shape[-1]
        N = _numel_spatial(p, 2)
        _, (pbs, pts) = _rows(p, 2)
        _, (gbs, gts) = _rows(g, 2)
        dpred = torch.empty(shape, dtype=torch.float32, device=p.device)
        L.call(
            "p4c_weighted_loss_bwd", L.ptr(gout.contiguous().float()), L.ptr(p), pbs, pts, L.ptr(g), gbs, gts,
            L.ptr(mtensor), mode, L.ptr(weights), L.ptr(interior), num_interior, L.ptr(count), kind, L.ptr(dpred),
            T * N * F, N * F, B, T, N, F, L.stream(p.device),
        )
        return dpred, None, None, None, None, None, None, None


def weighted_loss(pred, target, spec: MaskSpec, weights, interior, num_interior, kind, count=None):
    """losses.py:130-169 with reduce_spatial_dim=True -> (B,T)."""
    if count is None:
        count = masked_count(spec, target)
    return _WeightedLoss.apply(pred, target, spec, weights, interior, num_interior, count, kind)


def weighted_loss_map(pred, target, spec: MaskSpec, weights, kind):
    """losses.py:144-154 with reduce_spatial_dim=False -> (B,T,*S).  Not differentiable (plots only)."""
    L.require_cuda(pred, target)
    B, T, F = pred.shape[0], pred.shape[1], pred.shape[-1]
    N = _numel_spatial(pred, 2)
    p, (pbs, pts) = _rows(pred.detach().float(), 2)
    g, (gbs, gts) = _rows(target.detach().float(), 2)
    out = torch.empty(pred.shape[:-1], dtype=torch.float32, device=pred.device)
    L.call(
        "p4c_weighted_loss_map", L.ptr(p), pbs, pts, L.ptr(g), gbs, gts, L.ptr(spec.tensor), spec.mode, L.ptr(weights),
        kind, L.ptr(out), B, T, N, F, L.stream(pred.device),
    )
    return out


def scaled_loss(pred, target, spec: MaskSpec, std, interior, num_interior, kind, count=None):
    """losses.py:186-210 -> (B,T,F).  Metric path (val/test): not differentiable."""
    L.require_cuda(pred, target)
    B, T, F = pred.shape[0], pred.shape[1], pred.shape[-1]
    N = _numel_spatial(pred, 2)
    if count is None:
        count = masked_count(spec, target)
    p, (pbs, pts) = _rows(pred.detach().float(), 2)
    g, (gbs, gts) = _rows(target.detach().float(), 2)
    out = torch.empty(B, T, F, dtype=torch.float32, device=pred.device)
    ws = _workspace(B, T, N, F, pred.device)
    L.call(
        "p4c_scaled_loss_fwd", L.ptr(p), pbs, pts, L.ptr(g), gbs, gts, L.ptr(spec.tensor), spec.mode, L.ptr(std),
        L.ptr(interior), float(num_interior), L.ptr(count), kind, L.ptr(out), L.ptr(ws), B, T, N, F, L.stream(pred.device),
    )
    return out


def eval_sums(pred, target, spec: MaskSpec, std, interior, num_interior, weights, map_kind, map_acc=None, accumulate=False):
    """What the score-card and spatial-error observers need of one validation / test step, in one pass over prediction and target
    (p4c_eval_sums): returns ``(scores, masked_count)`` with ``scores`` (2,B,T,F) -- [0] = ``scaled_loss(..., L1)``, [1] =
    ``scaled_loss(..., MSE)`` -- and ``masked_count`` (1,) int32 = ``masked_count(spec, target)`` (0 without a mask).  With
    ``map_acc`` (T,*S) and ``map_kind`` (LOSS_MSE / LOSS_L1) the batch sum of ``weighted_loss_map`` is written to it
    (``accumulate=False``) or added to it (``accumulate=True``); ``map_kind=None`` forms no map.  Not differentiable."""
    L.require_cuda(pred, target)
    B, T, F = pred.shape[0], pred.shape[1], pred.shape[-1]
    N = _numel_spatial(pred, 2)
    p, (pbs, pts) = _rows(pred.detach().float(), 2)
    g, (gbs, gts) = _rows(target.detach().float(), 2)
    if map_kind is None:
        map_kind, map_acc = L.EVAL_MAP_NONE, None
    if map_acc is not None:
        if map_acc.dtype != torch.float32 or not map_acc.is_contiguous() or map_acc.numel() != T * N or map_acc.device != p.device:
            raise L.P4CError("eval_sums: map_acc must be a contiguous fp32 (T, *spatial) tensor on the prediction's device")
        if weights is None:
            raise L.P4CError("eval_sums: the map needs the per-feature weights")
    scores = torch.empty(2, B, T, F, dtype=torch.float32, device=p.device)
    count = torch.empty(1, dtype=torch.int32, device=p.device)
    ws = torch.empty(L.lib().p4c_eval_sums_workspace_bytes(B, T, N, F) // 4, dtype=torch.float32, device=p.device)
    L.call(
        "p4c_eval_sums", L.ptr(p), pbs, pts, L.ptr(g), gbs, gts, L.ptr(spec.tensor), spec.mode, L.ptr(interior), float(num_interior),
        L.ptr(std), L.ptr(weights), int(map_kind), L.ptr(map_acc), int(bool(accumulate)), L.ptr(scores), L.ptr(count), L.ptr(ws),
        B, T, N, F, L.stream(p.device),
    )
    return scores, count


# ------------------------------------------------------------------------------ K2+K3 fused training step
class _ARStepLoss(torch.autograd.Function):
    """
    One AR step of the training path: state update + that step's loss column in one pass.
    Inputs: prev (B,*S,F) or None, y (B,*S,y_cs) from the model, target (B,*S,F) = outputs[:, i].
    Outputs: new_state (B,*S,F) and loss (B,).
    """

    @staticmethod
    def forward(ctx, prev, y, target, std, mean, border_mask, interior_mask, weights, num_interior, count,
                kind, mask_mode, keep_prev, force_border, out=None):
        L.require_cuda(y, target)
        B, F = target.shape[0], target.shape[-1]
        y_c = y.contiguous()
        y_cs = y_c.shape[-1]
        N = _numel_spatial(target, 1)
        pv, pbs = (None, 0)
        if prev is not None:
            pv, (pbs,) = _rows(prev, 1)
        tg, (tbs,) = _rows(target, 1)
        if out is not None:   # caller-provided slot of the (B,T,*S,F) prediction buffer: no stack/copy afterwards
            assert out.shape == target.shape and out.dtype == torch.float32 and out[0].is_contiguous()
            new_state, nbs = out, out.stride(0)
        else:
            new_state, nbs = torch.empty(target.shape, dtype=torch.float32, device=y.device), N * F
        ns = new_state
        loss = torch.empty(B, dtype=torch.float32, device=y.device)
        ws = _workspace(B, 1, N, 1, y.device)
        L.call(
            "p4c_ar_update_loss_fwd", L.ptr(pv), pbs, L.ptr(y_c), L.dtype_code(y_c.dtype), y_cs, L.ptr(tg), tbs,
            L.ptr(std), L.ptr(mean), L.ptr(border_mask if force_border else None), L.ptr(interior_mask), L.ptr(ns), nbs,
            L.ptr(weights), float(num_interior), L.ptr(count), kind, mask_mode, L.ptr(loss), 1, L.ptr(ws), B, N, F,
            float(keep_prev), L.stream(y.device),
        )
        ctx.save_for_backward(ns, tg, std, interior_mask, weights, count)
        ctx.meta = (B, N, F, y_cs, y.dtype, nbs, tbs, float(num_interior), kind, mask_mode, float(keep_prev),
                    bool(force_border), prev is not None, prev.shape if prev is not None else None)
        return new_state, loss

    @staticmethod
    def backward(ctx, g_new, g_loss):
        ns, tg, std, interior, weights, count = ctx.saved_tensors
        B, N, F, y_cs, ydt, nbs, tbs, num_interior, kind, mask_mode, keep, force, has_prev, pshape = ctx.meta
        gn, gnbs = (None, 0)
        if g_new is not None:
            gn, (gnbs,) = _rows(g_new.float(), 1)
        gl = g_loss.contiguous().float() if g_loss is not None else None
        dy = torch.empty(tg.shape[:-1] + (y_cs,), dtype=ydt, device=tg.device)
        dprev = torch.empty(pshape, dtype=torch.float32, device=tg.device) if has_prev else None
        L.call(
            "p4c_ar_update_loss_bwd", L.ptr(gn), gnbs, None, L.dtype_code(ydt), 0, L.ptr(gl), 1, L.ptr(ns), nbs,
            L.ptr(tg), tbs, L.ptr(std), L.ptr(interior), int(force), L.ptr(weights), num_interior, L.ptr(count), kind,
            mask_mode, L.ptr(dy), L.dtype_code(ydt), y_cs, L.ptr(dprev), N * F, B, N, F, keep, L.stream(tg.device),
        )
        return (dprev, dy) + (None,) * 13


def ar_step_loss(prev, y, target, std, mean, border_mask, interior_mask, weights, num_interior, count, kind,
                 mask_mode, keep_prev, force_border, out=None):
    return _ARStepLoss.apply(prev, y, target, std, mean, border_mask, interior_mask, weights, num_interior,
                             count, kind, mask_mode, keep_prev, force_border, out)


# ------------------------------------------------------------------------------------------------ rows next to the path
def unnormalize(x: torch.Tensor, std: torch.Tensor, mean: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """out = x*std + mean per feature (last dim), as the reference's two in-place passes (lightning.py:1162-1169)."""
    L.require_cuda(x)
    x = x.contiguous().float()
    F = x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    L.call("p4c_unnormalize", L.ptr(x), L.ptr(std.to(x).contiguous()), L.ptr(mean.to(x).contiguous()), L.ptr(out),
           x.numel() // F, F, L.stream(x.device))
    return out


def unnormalize_planes(x: torch.Tensor, std: torch.Tensor, mean: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """x (B,T,*S,F) -> (B,T,F,*S): un-normalised, one contiguous plane per (sample, time step, feature) -- the layout the GRIB / GIF
    writers consume (io/outputs.py:116-241), same two rounded steps as ``unnormalize``."""
    L.require_cuda(x)
    x = x.contiguous().float()
    B, T, F = x.shape[0], x.shape[1], x.shape[-1]
    spatial = tuple(x.shape[2:-1])
    N = 1
    for d in spatial:
        N *= d
    if out is None:
        out = torch.empty((B, T, F) + spatial, dtype=torch.float32, device=x.device)
    L.call("p4c_unnormalize_planes", L.ptr(x), L.ptr(std.to(x).contiguous()), L.ptr(mean.to(x).contiguous()), L.ptr(out), B * T, N, F,
           L.stream(x.device))
    return out


def acc_sums(pred: torch.Tensor, target: torch.Tensor, spec: "MaskSpec", climate_means: torch.Tensor) -> torch.Tensor:
    """Spatial means of (p-c)(t-c)m, ((p-c)m)^2, ((t-c)m)^2 -> (3,B,T,F) (MetricACC.update, metrics.py:414-423)."""
    L.require_cuda(pred, target)
    p, g = pred.contiguous().float(), target.contiguous().float()
    B, T, F = p.shape[0], p.shape[1], p.shape[-1]
    N = p.numel() // (B * T * F)
    out = torch.empty(3, B, T, F, dtype=torch.float32, device=p.device)
    ws = torch.empty(3 * L.lib().p4c_loss_workspace_bytes(B, T, N, F) // 4, dtype=torch.float32, device=p.device)
    L.call("p4c_acc_sums", L.ptr(p), T * N * F, N * F, L.ptr(g), T * N * F, N * F, L.ptr(spec.tensor), spec.mode,
           L.ptr(climate_means.to(p).contiguous()), L.ptr(out), L.ptr(ws), B, T, N, F, L.stream(p.device))
    return out


@functools.lru_cache(maxsize=32)
def _psd_bins(H: int, W: int):
    """(Rmax, pixels per radial bin) of ``radial_bin_dct`` (metrics.py:300-318) for an (H, W) spectrum, as the reference has it:
    the centre (H//2, W//2) is used as (x0, y0) -- swapped for non-square grids -- and Rmax = min(W-1, H-1, r.max()) // 2."""
    y, x = np.indices((H, W))
    r = np.sqrt((x - H // 2) ** 2 + (y - W // 2) ** 2).astype(int)
    rmax = min(W - 1, H - 1, int(r.max())) // 2
    counts = np.bincount(r.ravel()[r.ravel() < rmax], minlength=rmax)[:rmax].astype(np.int32)
    counts.setflags(write=False)
    return rmax, counts


def psd_rmax(H: int, W: int) -> int:
    """Number of wave-number bins of the reference's power spectrum on an (H, W) grid."""
    return _psd_bins(int(H), int(W))[0]


def psd_bin_counts(H: int, W: int) -> np.ndarray:
    """(Rmax,) int32: pixels per radial bin; a bin with none is NaN in the spectrum (the reference's 0/0)."""
    return _psd_bins(int(H), int(W))[1]


@functools.lru_cache(maxsize=32)
def _psd_tables(H: int, W: int, device):
    h = np.arange(H, dtype=np.float64)
    col = np.cos(np.pi * (2 * h + 1) * (H - 1) / (2 * H)).astype(np.float32)   # row H-1 of the DCT-II basis along H
    return torch.from_numpy(col).to(device), torch.from_numpy(psd_bin_counts(H, W).copy()).to(device)


def psd(pred: torch.Tensor, target: torch.Tensor, spec: "MaskSpec", pred_step: int, grid=None) -> torch.Tensor:
    """Radially binned power spectral density of prediction and target at time step ``pred_step`` as the reference computes it
    (``power_spectral_density`` of metrics.py:324-352 on ``tensor * mask``, per feature) -> (2, F, Rmax), prediction first.
    (B,T,H,W,F) tensors, or (B,T,N,F) with ``grid=(H, W)``; one pass of ``p4c_psd`` over both tensors, nothing goes to the host."""
    L.require_cuda(pred, target)
    if pred.shape != target.shape:
        raise L.P4CError(f"psd: prediction {tuple(pred.shape)} and target {tuple(target.shape)} differ")
    if pred.dim() == 5 and grid is None:
        H, W = int(pred.shape[2]), int(pred.shape[3])
    elif pred.dim() == 4 and grid is not None:
        H, W = int(grid[0]), int(grid[1])
        if H * W != pred.shape[2]:
            raise L.P4CError(f"psd: grid {H}x{W} does not match {pred.shape[2]} grid points")
    else:
        raise L.P4CError("psd: needs (B,T,H,W,F) tensors, or (B,T,N,F) tensors with grid=(H, W)")
    B, T, F = pred.shape[0], pred.shape[1], pred.shape[-1]
    if not 0 <= pred_step < T:
        raise L.P4CError(f"psd: pred_step {pred_step} outside the {T} time steps")
    rmax = psd_rmax(H, W)
    if rmax < 1:
        raise L.P4CError(f"psd: a {H}x{W} grid has no wave-number bin (Rmax = 0)")
    p, (pbs, _) = _rows(pred.detach().float(), 2)
    g, (gbs, _) = _rows(target.detach().float(), 2)
    m, mbs = None, 0
    if spec.tensor is not None:
        m = spec.tensor
        if m.shape != pred.shape:
            m = m.expand(pred.shape).contiguous()
        m, mbs = m[:, pred_step], T * H * W * F
    col, counts = _psd_tables(H, W, p.device)
    out = torch.empty(2, F, rmax, dtype=torch.float32, device=p.device)
    ws = torch.empty(L.lib().p4c_psd_workspace_bytes(B, H, W, F) // 4, dtype=torch.float32, device=p.device)
    L.call("p4c_psd", L.ptr(p[:, pred_step]), pbs, L.ptr(g[:, pred_step]), gbs, L.ptr(m), mbs, spec.mode, L.ptr(col), L.ptr(counts),
           rmax, L.ptr(out), L.ptr(ws), B, H, W, F, L.stream(p.device), alg_bytes=2 * 4 * B * H * W * F)
    return out


def pack_standardize(raw: torch.Tensor, mean: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    """raw (F, *lead) parameter planes -> (*lead, F) standardised features-last tensor (base.py:448-452 + concat)."""
    L.require_cuda(raw)
    raw = raw.contiguous().float()
    F = raw.shape[0]
    rows = raw.numel() // F
    out = torch.empty(*raw.shape[1:], F, dtype=torch.float32, device=raw.device)
    L.call("p4c_pack_standardize", L.ptr(raw), rows, L.ptr(mean.to(raw).contiguous()), L.ptr(std.to(raw).contiguous()),
           L.ptr(out), rows, F, L.stream(raw.device))
    return out


def build_forcing(raw, mean, std, table: torch.Tensor, grid_planes: torch.Tensor, B: int, T: int, H: int, W: int) -> torch.Tensor:
    """The forcing batch of ``Sample.load`` (base.py:455-527) in one pass of ``p4c_build_forcing`` -> (B, T, H, W, Fe + 5) fp32:
    ``raw`` (Fe, B, T, H, W) external forcing planes (or None: Fe = 0) standardised and packed as ``pack_standardize`` does,
    then the reference's five generated channels (``forcings.FORCING_NAMES``).  ``table``: (B, T, 8) of ``forcings.time_table``,
    ``grid_planes``: (3, H, W) of ``forcings.grid_tables``, both on the device."""
    L.require_cuda(raw, table, grid_planes)
    B, T, H, W = int(B), int(T), int(H), int(W)
    if tuple(table.shape) != (B, T, 8) or tuple(grid_planes.shape) != (3, H, W):
        raise L.P4CError(f"build_forcing: table {tuple(table.shape)} / grid planes {tuple(grid_planes.shape)} do not match "
                         f"(B, T, 8) = {(B, T, 8)} and (3, H, W) = {(3, H, W)}")
    dev = table.device
    table = table.contiguous().float()
    planes = grid_planes.to(dev).contiguous().float()
    Fe, rows = 0, B * T * H * W
    if raw is not None:
        if raw.dim() != 5 or tuple(raw.shape[1:]) != (B, T, H, W):
            raise L.P4CError(f"build_forcing: raw {tuple(raw.shape)} is not (Fe, B, T, H, W) = (Fe, {B}, {T}, {H}, {W})")
        raw = raw.to(dev).contiguous().float()
        Fe = raw.shape[0]
        if mean.numel() != Fe or std.numel() != Fe:
            raise L.P4CError(f"build_forcing: {Fe} external features, {mean.numel()} means, {std.numel()} standard deviations")
        mean, std = mean.to(raw).contiguous(), std.to(raw).contiguous()
    if Fe == 0:
        raw = mean = std = None
    out = torch.empty(B, T, H, W, Fe + 5, dtype=torch.float32, device=dev)
    L.call("p4c_build_forcing", L.ptr(raw), rows, L.ptr(mean), L.ptr(std), L.ptr(planes[0]), L.ptr(planes[1]), L.ptr(planes[2]),
           L.ptr(table), L.ptr(out), B, T, H * W, Fe, L.stream(dev), alg_bytes=4 * rows * (2 * Fe + 5))
    return out


# host mirrors of p4c_regrid_tap / p4c_regrid_feature (include/py4cast_hip.h)
REGRID_TAP = np.dtype([("i0", "<i4"), ("i1", "<i4"), ("f", "<f4"), ("pad", "<i4")])
REGRID_FEATURE = np.dtype([("src", "<u8"), ("b_stride", "<i8"), ("t_stride", "<i8"), ("pitch", "<i4"), ("row0", "<i4"), ("col0", "<i4"),
                           ("table", "<i4"), ("mean", "<f4"), ("std", "<f4"), ("channel", "<i4"), ("pad", "<i4")])
REGRID_MAX_FEATURES = 144


def planes_dense(t: torch.Tensor) -> bool:
    """every (H, W) plane of ``t`` (..., H, W) is dense; the strides of the leading dimensions are free (planes at a pitch)"""
    return t.is_contiguous() or (t.dim() >= 2 and t.stride(-1) == 1 and t.stride(-2) == t.shape[-1])


def regrid_features(sources, feats, table_dims, B: int, T: int) -> torch.Tensor:
    """The device descriptors (p4c_regrid_feature) of ``regrid_pack``, checked on the host: everything the kernel will index lies
    inside its plane, and the output channels are 0 .. F-1, each once.

    sources: device tensors (Fg, B, T, Hs, Ws) fp32, every plane dense (``planes_dense``: the planes may lie at a pitch).  feats: one tuple per output feature, (index into sources, plane of
    that source, window row origin, window column origin, tap table, mean, std, output channel).  table_dims: per tap table the
    (rows, columns) of the windowed source it indexes.  The result holds raw pointers into ``sources``: keep them alive."""
    L.require_cuda(*sources)
    F = len(feats)
    if not 1 <= F <= REGRID_MAX_FEATURES:
        raise L.P4CError(f"regrid_pack: {F} features: 1 .. at most {REGRID_MAX_FEATURES} per call (LDS tile)")
    dev = sources[0].device
    for s in sources:
        if s.dim() != 5 or tuple(s.shape[1:3]) != (B, T) or s.dtype != torch.float32 or not planes_dense(s) or s.device != dev:
            raise L.P4CError(f"regrid_pack: source {tuple(s.shape)} {s.dtype} is not a dense fp32 (Fg, {B}, {T}, Hs, Ws) on {dev}")
    if sorted(f[7] for f in feats) != list(range(F)):
        raise L.P4CError(f"regrid_pack: the output channels {sorted(f[7] for f in feats)} are not 0 .. {F - 1}, each once")
    desc = np.zeros(F, dtype=REGRID_FEATURE)
    for i, (si, plane, row0, col0, table, mean, std, channel) in enumerate(feats):
        s = sources[si]
        Fg, _, _, Hs, Ws = s.shape
        if not (0 <= plane < Fg and 0 <= table < len(table_dims)):
            raise L.P4CError(f"regrid_pack: feature {i}: plane {plane} of {Fg}, tap table {table} of {len(table_dims)}")
        n, m = table_dims[table]
        if not (0 <= row0 and row0 + n <= Hs and 0 <= col0 and col0 + m <= Ws):
            raise L.P4CError(f"regrid_pack: feature {i}: window {n} x {m} at ({row0}, {col0}) leaves its {Hs} x {Ws} plane")
        desc[i] = (s.data_ptr() + 4 * plane * s.stride(0), s.stride(1), s.stride(2), Ws, row0, col0, table, mean, std, channel, 0)
    return torch.from_numpy(desc.view(np.uint8)).to(dev)


def regrid_pack(sources, feats, taps: torch.Tensor, table_dims, B: int, T: int, H: int, W: int, src_bytes: int = 0) -> torch.Tensor:
    """Native-grid planes -> (B, T, H, W, F) fp32 standardised features-last on the sub-domain, one pass of ``p4c_regrid_pack``
    (``py4cast_amd/regrid.py`` has the definition and builds the tables).

    sources, feats, table_dims: as ``regrid_features`` takes them; ``feats`` may also be the tensor it returned for these very
    sources (a caller that launches more than once on the same planes).  taps: (tables, H + W, 4) int32 on the device
    (``regrid.device_taps``).  src_bytes: the algorithmic bytes read from the sources (``regrid.source_bytes``)."""
    L.require_cuda(taps, *sources)
    B, T, H, W = int(B), int(T), int(H), int(W)
    if taps.dtype != torch.int32 or taps.dim() != 3 or tuple(taps.shape[1:]) != (H + W, 4) or taps.shape[0] != len(table_dims):
        raise L.P4CError(f"regrid_pack: taps {tuple(taps.shape)} {taps.dtype} are not ({len(table_dims)}, H + W = {H + W}, 4) int32")
    feats_dev = feats if isinstance(feats, torch.Tensor) else regrid_features(sources, feats, table_dims, B, T)
    F = feats_dev.numel() // REGRID_FEATURE.itemsize
    dev = taps.device
    if feats_dev.device != dev or feats_dev.dtype != torch.uint8 or feats_dev.numel() != F * REGRID_FEATURE.itemsize or F < 1:
        raise L.P4CError(f"regrid_pack: descriptors {tuple(feats_dev.shape)} {feats_dev.dtype} on {feats_dev.device}: not regrid_features' on {dev}")
    out = torch.empty(B, T, H, W, F, dtype=torch.float32, device=dev)
    L.call("p4c_regrid_pack", L.ptr(feats_dev), L.ptr(taps), L.ptr(out), B, T, H, W, F, L.stream(dev),
           alg_bytes=int(src_bytes) + 4 * out.numel())
    return out


# host mirror of p4c_convert_feature (include/py4cast_hip.h)
CONVERT_FEATURE = np.dtype([("src", "<u8"), ("b_stride", "<i8"), ("t_stride", "<i8"), ("floor", "<f4"), ("div", "<f4"), ("mul", "<f4"),
                            ("mean", "<f4"), ("std", "<f4"), ("flags", "<i4"), ("channel", "<i4"), ("pad", "<i4")])
CONVERT_FLIP_ROWS, CONVERT_HAS_FLOOR = 1, 2
CONVERT_MAX_FEATURES = 144


def convert_dtype_code(dt: torch.dtype) -> int:
    """the P4C_SRC_* code of a source dtype (``p4c_pack_convert`` reads u8, i16, u16, i32, f16, f32 and f64 planes)"""
    codes = {torch.uint8: 0, torch.int16: 1, torch.uint16: 2, torch.int32: 3, torch.float16: 4, torch.float32: 5, torch.float64: 6}
    if dt not in codes:
        raise L.P4CError(f"pack_convert: source dtype {dt} is none of {', '.join(str(k) for k in codes)}")
    return codes[dt]


def convert_features(sources, feats, B: int, T: int, H: int, W: int):
    """The device descriptors (p4c_convert_feature) of ``pack_convert``, checked on the host -> (descriptors, vec).

    sources: device tensors (Fg, B, T, H, W), all of ONE dtype of ``convert_dtype_code``, every plane dense (``planes_dense``: the
    strides of the three leading dimensions are free, so planes may lie at a pitch).  feats: one tuple per output feature,
    (index into sources, plane of that source, floor or None, div, mul, flip_rows, mean, std, output channel).  A feature's first
    plane must start on a 16-byte boundary (a torch allocation or a padded slot of a pinned buffer does).  vec: whether every
    16 bytes of a source row can be one load -- W and all batch / step strides are multiples of 16 / itemsize.  The result
    holds raw pointers into ``sources``: keep them alive."""
    L.require_cuda(*sources)
    F = len(feats)
    if not 1 <= F <= CONVERT_MAX_FEATURES:
        raise L.P4CError(f"pack_convert: {F} features: 1 .. at most {CONVERT_MAX_FEATURES} per call (LDS tile)")
    if int(B) * int(T) * int(H) * int(W) >= 1 << 31:
        raise L.P4CError(f"pack_convert: {int(B) * int(T) * int(H) * int(W)} rows: at most 2^31 - 1 per call")
    if not sources:
        raise L.P4CError("pack_convert: no sources")
    dev, dt = sources[0].device, sources[0].dtype
    convert_dtype_code(dt)
    size = sources[0].element_size()
    per = 16 // size
    for s in sources:
        if s.dim() != 5 or tuple(s.shape[1:]) != (B, T, H, W) or s.dtype != dt or not planes_dense(s) or s.device != dev:
            raise L.P4CError(f"pack_convert: source {tuple(s.shape)} {s.dtype} is not a dense {dt} (Fg, {B}, {T}, {H}, {W}) on {dev}")
        if min(s.stride()[:3]) < 0:
            raise L.P4CError(f"pack_convert: source strides {s.stride()} are negative")
    if sorted(f[8] for f in feats) != list(range(F)):
        raise L.P4CError(f"pack_convert: the output channels {sorted(f[8] for f in feats)} are not 0 .. {F - 1}, each once")
    desc = np.zeros(F, dtype=CONVERT_FEATURE)
    vec = W % per == 0
    for i, (si, plane, floor, div, mul, flip, mean, std, channel) in enumerate(feats):
        if not 0 <= si < len(sources):
            raise L.P4CError(f"pack_convert: feature {i}: source {si} of {len(sources)}")
        s = sources[si]
        if not 0 <= plane < s.shape[0]:
            raise L.P4CError(f"pack_convert: feature {i}: plane {plane} of {s.shape[0]}")
        base = s.data_ptr() + size * plane * s.stride(0)
        if base % 16:
            raise L.P4CError(f"pack_convert: feature {i}: its first plane starts at address {base:#x}, not on a 16-byte boundary")
        bs, ts = (s.stride(1) if B > 1 else 0), (s.stride(2) if T > 1 else 0)
        vec = vec and bs % per == 0 and ts % per == 0
        flags = (CONVERT_FLIP_ROWS if flip else 0) | (CONVERT_HAS_FLOOR if floor is not None else 0)
        desc[i] = (base, bs, ts, 0.0 if floor is None else floor, div, mul, mean, std, flags, channel, 0)
    return torch.from_numpy(desc.view(np.uint8)).to(dev), bool(vec)


def pack_convert(sources, feats, B: int, T: int, H: int, W: int) -> torch.Tensor:
    """Planes in the files' own dtype -> (B, T, H, W, F) fp32 standardised features-last, one pass of ``p4c_pack_convert``:
    ``(float)raw``, the floor, ``/ div``, ``* mul`` (each a rounded fp32 step, a factor of exactly 1 skipped), the row flip, then
    ``(v - mean) / std`` as ``pack_standardize`` does.  sources, feats: as ``convert_features`` takes them (and checks them)."""
    B, T, H, W = int(B), int(T), int(H), int(W)
    feats_dev, vec = convert_features(sources, feats, B, T, H, W)
    return pack_convert_launch(sources, feats_dev, vec, B, T, H, W)


def pack_convert_launch(sources, feats_dev: torch.Tensor, vec: bool, B: int, T: int, H: int, W: int) -> torch.Tensor:
    """the launch of ``pack_convert`` on descriptors ``convert_features`` made for these very sources and dimensions"""
    F = feats_dev.numel() // CONVERT_FEATURE.itemsize
    dev, dt = sources[0].device, sources[0].dtype
    if feats_dev.device != dev or feats_dev.dtype != torch.uint8 or feats_dev.numel() != F * CONVERT_FEATURE.itemsize or F < 1:
        raise L.P4CError(f"pack_convert: descriptors {tuple(feats_dev.shape)} {feats_dev.dtype} on {feats_dev.device}: not convert_features' on {dev}")
    out = torch.empty(B, T, H, W, F, dtype=torch.float32, device=dev)
    L.call("p4c_pack_convert", L.ptr(feats_dev), L.ptr(out), convert_dtype_code(dt), int(vec), B, T, H, W, F, L.stream(dev),
           alg_bytes=(sources[0].element_size() + 4) * out.numel())
    return out


def regrid_blur(src: torch.Tensor, window, row_index: torch.Tensor, col_index: torch.Tensor, row_w: torch.Tensor,
                col_w: torch.Tensor) -> torch.Tensor:
    """The Gaussian of ``resize(anti_aliasing=True)`` over the window (r0, r1, c0, c1) of every plane of ``src`` (..., Hs, Ws) ->
    dense (..., n, m) fp32, ``scipy.ndimage.gaussian_filter(mode="mirror")`` axis 0 then axis 1 (``p4c_regrid_blur``).  row_index:
    (n + 2 ry) int32 mirrored source rows of the positions -ry .. n - 1 + ry, row_w: (2 ry + 1) weights; columns likewise
    (``regrid.device_blur_tables``)."""
    L.require_cuda(src, row_index, col_index, row_w, col_w)
    if src.dim() < 2:
        raise L.P4CError(f"regrid_blur: src {tuple(src.shape)} is not (..., Hs, Ws)")
    src = src.contiguous().float()
    Hs, Ws = src.shape[-2:]
    r0, r1, c0, c1 = (int(v) for v in window)
    n, m = r1 - r0, c1 - c0
    if not (0 <= r0 and r1 <= Hs and 0 <= c0 and c1 <= Ws):
        raise L.P4CError(f"regrid_blur: window {(r0, r1, c0, c1)} does not lie inside planes of {Hs} x {Ws}")
    if n < 2 or m < 2:
        raise L.P4CError(f"regrid_blur: a {n} x {m} window: each axis needs at least 2 points")
    ry, rx = (row_w.numel() - 1) // 2, (col_w.numel() - 1) // 2
    if row_w.numel() != 2 * ry + 1 or col_w.numel() != 2 * rx + 1 or ry > 64 or rx > 64:
        raise L.P4CError(f"regrid_blur: {row_w.numel()} / {col_w.numel()} weights: an odd count, radius at most 64")
    if row_index.numel() != n + 2 * ry or col_index.numel() != m + 2 * rx or row_index.dtype != torch.int32 or col_index.dtype != torch.int32:
        raise L.P4CError(f"regrid_blur: index tables of {row_index.numel()} / {col_index.numel()} {row_index.dtype} entries, "
                         f"expected int32 of {n + 2 * ry} / {m + 2 * rx}")
    planes = src.numel() // (Hs * Ws)
    out = torch.empty(*src.shape[:-2], n, m, dtype=torch.float32, device=src.device)
    L.call("p4c_regrid_blur", L.ptr(src), Hs * Ws, Ws, r0, c0, L.ptr(out), planes, n, m, L.ptr(row_index.contiguous()),
           L.ptr(col_index.contiguous()), L.ptr(row_w.contiguous().float()), ry, L.ptr(col_w.contiguous().float()), rx, L.stream(src.device),
           alg_bytes=4 * planes * 2 * n * m)
    return out


# ------------------------------------------------------------------------------------------------ prediction maps
# launch constants of csrc/map_frames.hip (the library reports the same through p4c_map_tile() etc.): a test sizes a case past
# one loop trip from them
MAP_TILE = 256                # grid points per loop trip of a map_planes workgroup
MAP_MAX_BLOCKS = 512          # workgroups of one map_planes launch, all samples together
MAP_MAX_FEATURES = 256        # K of one map_planes call
MAP_GAP = 8                   # white columns between the target and the prediction panel of a frame
MAP_RENDER_PIXELS = 4         # pixels per thread (256 per workgroup) and loop trip of map_render
MAP_RENDER_MAX_BLOCKS = 512   # workgroups of one map_render launch


@functools.lru_cache(maxsize=32)
def _map_feature_index(features: tuple, device_index: int) -> torch.Tensor:
    return torch.tensor(features, dtype=torch.int32, device=torch.device("cuda", device_index))


def map_planes(pred, target, spec: MaskSpec, std, mean, features, n: int):
    """Prediction and target (B,T,*S,F) -> the planes the map observers draw, of the ``n`` leading samples and the features
    ``features`` (indices into F) only (p4c_map_planes): ``planes`` (n,T,K,2,N) fp32 with [..., 0, :] = ``target*std+mean`` and
    [..., 1, :] = ``(pred*mask)*std+mean`` -- the two / three separately rounded fp32 steps of plots.py:271, 299-300 -- and
    ``vrange`` (n,K,2), min and max of panel 0 over (T,N) (plots.py:311-312; NaN propagates).  ``spec`` as for ``eval_sums``; with
    MASK_FROM_NAN ``target`` is the raw target and its NaNs count as 0.  Not differentiable."""
    L.require_cuda(pred, target, std, mean)
    if pred.dim() < 4 or pred.shape != target.shape:
        raise L.P4CError(f"map_planes: prediction {tuple(pred.shape)} / target {tuple(target.shape)}: equal (B, T, *spatial, F) expected")
    B, T, F = pred.shape[0], pred.shape[1], pred.shape[-1]
    N = _numel_spatial(pred, 2)
    features = tuple(int(f) for f in features)
    K, n = len(features), int(n)
    if not 1 <= n <= B:
        raise L.P4CError(f"map_planes: n = {n} samples of a batch of {B}")
    if not 1 <= K <= MAP_MAX_FEATURES:
        raise L.P4CError(f"map_planes: {K} features: 1 .. at most {MAP_MAX_FEATURES} per call")
    if min(features) < 0 or max(features) >= F:
        raise L.P4CError(f"map_planes: feature indices {features} leave 0 .. {F - 1}")
    if std.numel() != F or mean.numel() != F:
        raise L.P4CError(f"map_planes: {std.numel()} standard deviations / {mean.numel()} means for {F} features")
    if spec.mode in (L.MASK_F32, L.MASK_U8):
        if spec.tensor is None or spec.tensor.numel() != pred.numel() or not spec.tensor.is_contiguous() or spec.tensor.device != pred.device:
            raise L.P4CError("map_planes: an explicit mask is a dense tensor of the prediction's shape on its device")
    p, (pbs, pts) = _rows(pred.detach().float(), 2)
    g, (gbs, gts) = _rows(target.detach().float(), 2)
    dev = p.device
    std, mean = std.to(p).contiguous(), mean.to(p).contiguous()
    planes = torch.empty(n, T, K, 2, N, dtype=torch.float32, device=dev)
    vrange = torch.empty(n, K, 2, dtype=torch.float32, device=dev)
    ws = torch.empty(L.lib().p4c_map_planes_workspace_bytes(n, T, N, K) // 4, dtype=torch.float32, device=dev)
    index = _map_feature_index(features, dev.index if dev.index is not None else torch.cuda.current_device())
    L.call(
        "p4c_map_planes", L.ptr(p), pbs, pts, L.ptr(g), gbs, gts, L.ptr(spec.tensor), spec.mode, L.ptr(std), L.ptr(mean), L.ptr(index),
        L.ptr(planes), L.ptr(vrange), L.ptr(ws), n, T, N, F, K, L.stream(dev),
        alg_bytes=n * T * N * K * (2 * 64 + 2 * 4),   # a 64-byte line per point and tensor where the K features share one
    )
    return planes, vrange


def map_render(planes, vrange, lut, interior, H: int, W: int, out: torch.Tensor = None) -> torch.Tensor:
    """``map_planes``' results -> RGB8 frames (n,T,K,H,2W+MAP_GAP,3) (p4c_map_render): the target panel left, the prediction
    right, MAP_GAP white columns between, grid row 0 at the bottom.  ``lut``: (256,3) uint8 colour table; ``interior``: the
    (H*W,) interior mask, the border fades to ``clamp(interior, 0.7, 1)`` over white (plots.py:134).  The colour index is
    matplotlib's: 0 below the range, 255 from its top, else floor(256 (v-vmin)/(vmax-vmin)); NaN is white.  ``out``: a dense uint8 device tensor of the
    frames' shape at a 4-byte aligned address to render into (a caller that ships frames and ranges in one buffer)."""
    L.require_cuda(planes, vrange, lut, interior)
    H, W = int(H), int(W)
    if planes.dim() != 5 or planes.shape[3] != 2 or planes.dtype != torch.float32 or not planes.is_contiguous():
        raise L.P4CError(f"map_render: planes {tuple(planes.shape)} {planes.dtype}: a dense fp32 (n, T, K, 2, N) expected")
    n, T, K, _, N = planes.shape
    if H < 1 or W < 1 or H * W != N:
        raise L.P4CError(f"map_render: a {H} x {W} grid for planes of {N} points")
    if tuple(vrange.shape) != (n, K, 2) or vrange.dtype != torch.float32 or not vrange.is_contiguous():
        raise L.P4CError(f"map_render: vrange {tuple(vrange.shape)} {vrange.dtype}: a dense fp32 ({n}, {K}, 2) expected")
    if tuple(lut.shape) != (256, 3) or lut.dtype != torch.uint8 or not lut.is_contiguous():
        raise L.P4CError(f"map_render: colour table {tuple(lut.shape)} {lut.dtype}: a dense uint8 (256, 3) expected")
    if interior.numel() != N:
        raise L.P4CError(f"map_render: an interior mask of {interior.numel()} points for planes of {N}")
    RW = 2 * W + MAP_GAP
    if n * T * K * H * RW >= 2 ** 31:
        raise L.P4CError(f"map_render: {n * T * K * H * RW} pixels: fewer than 2^31 per call")
    interior = interior.reshape(-1).to(planes).contiguous()
    shape = (n, T, K, H, RW, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=planes.device)
    elif (tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != planes.device
          or out.data_ptr() % 4):
        raise L.P4CError(f"map_render: out {tuple(out.shape)} {out.dtype}: a dense, 4-byte aligned uint8 {shape} on {planes.device} expected")
    frames = out
    L.call("p4c_map_render", L.ptr(planes), L.ptr(vrange), L.ptr(lut), L.ptr(interior), L.ptr(frames), n, T, K, H, W,
           L.stream(planes.device), alg_bytes=planes.numel() * 4 + frames.numel())
    return frames


# ------------------------------------------------------------------------------------------------ forecast frames
# launch constants of csrc/forecast_frames.hip (p4c_forecast_tile() etc. report the same)
FORECAST_TILE = 128            # grid points per loop trip of a workgroup
FORECAST_MAX_BLOCKS = 1024     # workgroups of one launch, all (sample, lead time) pairs together
FORECAST_MAX_FEATURES = 256    # K of one call
FORECAST_MAX_SAMPLES = 256     # n of one call
FORECAST_BAD = 255             # the palette index of a pixel that is not drawn


def _display_row(d) -> tuple:
    """(offset, floor, vmin, vmax) of one feature as floats: from an object with these attributes (outputs.FeatureDisplay) or a
    4-tuple; None = no offset / no floor / auto-scaled"""
    if not isinstance(d, (tuple, list)):
        d = (d.offset, d.floor, d.vmin, d.vmax)
    off, flo, lo, hi = d
    row = (0.0 if off is None else float(off), float("-inf") if flo is None else float(flo),
           float("nan") if lo is None else float(lo), float("nan") if hi is None else float(hi))
    if row[0] != row[0] or abs(row[0]) == float("inf") or abs(row[2]) == float("inf") or abs(row[3]) == float("inf"):
        raise L.P4CError(f"forecast_frames: display row {d}: a finite offset, and a finite or absent (auto-scaled) range expected")
    return row


@functools.lru_cache(maxsize=32)
def _forecast_tables(features: tuple, rows: tuple, device_index: int):
    dev = torch.device("cuda", device_index)
    return (torch.tensor(features, dtype=torch.int32, device=dev), torch.tensor(rows, dtype=torch.float32, device=dev).reshape(-1, 4),
            any(r[2] != r[2] or r[3] != r[3] for r in rows))


def forecast_frames(pred, std, mean, display, samples=None, features=None, out=None):
    """The normalised prediction (B,T,H,W,F) -- or (B,T,N,F), one row of N pixels -- -> palette-index frames (p4c_forecast_frames):
    ``frames`` (n,T,K,H,W) uint8, grid row 0 at the bottom, and ``vrange`` (n,T,K,2) fp32, the colour range of every frame.
    ``display``: one row (offset, floor, vmin, vmax) per feature of F (tuples, or objects with these attributes; None = none /
    auto-scaled per frame); ``samples``: indices into B (default all); ``features``: indices into F to draw (default all).
    A pixel is ``v = pred*std + mean (+ offset)``; it gets FORECAST_BAD = 255 when v is not finite or below the floor, else 0 ..
    254 by matplotlib's Normalize rule over 255 colours.  ``out``: (frames, vrange) dense device tensors of those shapes to write
    into, frames 4-byte aligned.  Not differentiable."""
    L.require_cuda(pred, std, mean)
    if pred.dim() not in (4, 5):
        raise L.P4CError(f"forecast_frames: prediction {tuple(pred.shape)}: (B, T, H, W, F) or (B, T, N, F) expected")
    B, T, F = pred.shape[0], pred.shape[1], pred.shape[-1]
    H, W = (pred.shape[2], pred.shape[3]) if pred.dim() == 5 else (1, pred.shape[2])
    display = list(display)
    if len(display) != F or std.numel() != F or mean.numel() != F:
        raise L.P4CError(f"forecast_frames: {len(display)} display rows / {std.numel()} standard deviations / {mean.numel()} means "
                         f"for {F} features")
    features = tuple(range(F)) if features is None else tuple(int(f) for f in features)
    samples = tuple(range(B)) if samples is None else tuple(int(s) for s in samples)
    K, n = len(features), len(samples)
    if not 1 <= K <= FORECAST_MAX_FEATURES:
        raise L.P4CError(f"forecast_frames: {K} features: 1 .. at most {FORECAST_MAX_FEATURES} per call")
    if min(features) < 0 or max(features) >= F:
        raise L.P4CError(f"forecast_frames: feature indices {features} leave 0 .. {F - 1}")
    if not 1 <= n <= FORECAST_MAX_SAMPLES or n * T > 65535:
        raise L.P4CError(f"forecast_frames: {n} samples: 1 .. at most {FORECAST_MAX_SAMPLES} per call, n*T <= 65535")
    if min(samples) < 0 or max(samples) >= B:
        raise L.P4CError(f"forecast_frames: sample indices {samples} leave 0 .. {B - 1}")
    N = H * W
    if n * T * K * N >= 2 ** 31:
        raise L.P4CError(f"forecast_frames: {n * T * K * N} pixels: fewer than 2^31 per call")
    p, (pbs, pts) = _rows(pred.detach().float(), 2)
    dev = p.device
    std, mean = std.to(p).contiguous(), mean.to(p).contiguous()
    rows = tuple(_display_row(display[f]) for f in features)
    index, table, auto = _forecast_tables(features, rows, dev.index if dev.index is not None else torch.cuda.current_device())
    fshape, rshape = (n, T, K, H, W), (n, T, K, 2)
    if out is None:
        frames = torch.empty(fshape, dtype=torch.uint8, device=dev)
        vrange = torch.empty(rshape, dtype=torch.float32, device=dev)
    else:
        frames, vrange = out
        if (tuple(frames.shape) != fshape or frames.dtype != torch.uint8 or not frames.is_contiguous() or frames.device != dev
                or frames.data_ptr() % 4 or tuple(vrange.shape) != rshape or vrange.dtype != torch.float32
                or not vrange.is_contiguous() or vrange.device != dev):
            raise L.P4CError(f"forecast_frames: out: a dense, 4-byte aligned uint8 {fshape} and a dense fp32 {rshape} on {dev} expected")
    ws = torch.empty(L.lib().p4c_forecast_frames_workspace_bytes(n, T, N, K) // 4, dtype=torch.float32, device=dev) if auto else None
    host_samples = (ctypes.c_int32 * n)(*samples)
    dense = bool(L.lib().p4c_forecast_frames_dense(K, F))
    per_point = 4 * F if dense else 64 * K   # whole points, or a 64-byte line per drawn feature where no two share one
    L.call("p4c_forecast_frames", L.ptr(p), pbs, pts, host_samples, L.ptr(std), L.ptr(mean), L.ptr(index), L.ptr(table), int(auto),
           L.ptr(frames), L.ptr(vrange), L.ptr(ws), B, n, T, H, W, F, K, L.stream(dev),
           alg_bytes=n * T * N * ((2 if auto else 1) * per_point + K))
    return frames, vrange


# ------------------------------------------------------------------------------------------------ GRIB2 simple packing
# launch constants of csrc/grib_pack.hip (p4c_grib_tile() etc. report the same)
GRIB_TILE = 128                # points per loop trip of a workgroup
GRIB_MAX_BLOCKS = 1024         # workgroups of one launch, all (sample, lead time) pairs together
GRIB_MAX_FEATURES = 256        # K of one call
GRIB_MAX_SAMPLES = 256         # n of one call
GRIB_PARAMS = 5                # int32 words of a params record: vmin, vmax, R (fp32 bits), E, bad


@functools.lru_cache(maxsize=32)
def _grib_features(features: tuple, device_index: int):
    return torch.tensor(features, dtype=torch.int32, device=torch.device("cuda", device_index))


def grib_pitch(N: int, spec) -> int:
    """bytes between two fields of ``grib_pack``'s ``packed``: the longest stream, ceil(N nbits / 8), rounded up to a multiple of 4"""
    return (max((N * int(nbits) + 7) // 8 for _, nbits in spec) + 3) // 4 * 4


def grib_pack(pred, std, mean, spec, samples=None, features=None, flip_rows=False, out=None):
    """The normalised prediction (B,T,H,W,F) -- or (B,T,N,F), one row of N points -- -> GRIB2 simple packing (p4c_grib_pack):
    ``params`` (n,T,K,5) int32 -- vmin, vmax, R as the bits of fp32 values, E, bad -- and ``packed`` (n,T,K,pitch) uint8, of which the
    first ceil(N nbits / 8) bytes of a row are the field's bit stream (``grib_pitch``).  ``spec``: one (D, nbits) per PACKED feature;
    ``samples``: indices into B (default all); ``features``: indices into F to pack (default all); ``flip_rows``: stream row r holds
    grid row H-1-r.  A value is ``v = pred*std + mean``, then X = min(floor((v 10^D - R) / 2^E + 0.5), 2^nbits - 1) in float64 with R
    the largest fp32 below the field's scaled minimum and E the smallest exponent that fits its range (include/py4cast_hip.h).
    ``out``: (params, packed) dense device tensors of those shapes to write into, packed 4-byte aligned.  Not differentiable."""
    L.require_cuda(pred, std, mean)
    if pred.dim() not in (4, 5):
        raise L.P4CError(f"grib_pack: prediction {tuple(pred.shape)}: (B, T, H, W, F) or (B, T, N, F) expected")
    B, T, F = pred.shape[0], pred.shape[1], pred.shape[-1]
    H, W = (pred.shape[2], pred.shape[3]) if pred.dim() == 5 else (1, pred.shape[2])
    if std.numel() != F or mean.numel() != F:
        raise L.P4CError(f"grib_pack: {std.numel()} standard deviations / {mean.numel()} means for {F} features")
    features = tuple(range(F)) if features is None else tuple(int(f) for f in features)
    samples = tuple(range(B)) if samples is None else tuple(int(s) for s in samples)
    spec = [(int(D), int(nbits)) for D, nbits in spec]
    K, n = len(features), len(samples)
    if not 1 <= K <= GRIB_MAX_FEATURES:
        raise L.P4CError(f"grib_pack: {K} features: 1 .. at most {GRIB_MAX_FEATURES} per call")
    if len(spec) != K:
        raise L.P4CError(f"grib_pack: {len(spec)} (D, nbits) pairs for {K} packed features")
    if min(features) < 0 or max(features) >= F:
        raise L.P4CError(f"grib_pack: feature indices {features} leave 0 .. {F - 1}")
    if not 1 <= n <= GRIB_MAX_SAMPLES or n * T > 65535:
        raise L.P4CError(f"grib_pack: {n} samples: 1 .. at most {GRIB_MAX_SAMPLES} per call, n*T <= 65535")
    if min(samples) < 0 or max(samples) >= B:
        raise L.P4CError(f"grib_pack: sample indices {samples} leave 0 .. {B - 1}")
    if any(abs(D) > 15 or not 1 <= nbits <= 32 for D, nbits in spec):
        raise L.P4CError(f"grib_pack: spec {spec}: |D| <= 15 and 1 <= nbits <= 32 expected")
    N = H * W
    pitch = grib_pitch(N, spec)
    if n * T * K * pitch >= 2 ** 31:
        raise L.P4CError(f"grib_pack: {n * T * K * pitch} stream bytes: fewer than 2^31 per call")
    p, (pbs, pts) = _rows(pred.detach().float(), 2)
    dev = p.device
    std, mean = std.to(p).contiguous(), mean.to(p).contiguous()
    index = _grib_features(features, dev.index if dev.index is not None else torch.cuda.current_device())
    pshape, sshape = (n, T, K, GRIB_PARAMS), (n, T, K, pitch)
    if out is None:
        params = torch.empty(pshape, dtype=torch.int32, device=dev)
        packed = torch.empty(sshape, dtype=torch.uint8, device=dev)
    else:
        params, packed = out
        if (tuple(params.shape) != pshape or params.dtype != torch.int32 or not params.is_contiguous() or params.device != dev
                or tuple(packed.shape) != sshape or packed.dtype != torch.uint8 or not packed.is_contiguous() or packed.device != dev
                or packed.data_ptr() % 4):
            raise L.P4CError(f"grib_pack: out: a dense int32 {pshape} and a dense, 4-byte aligned uint8 {sshape} on {dev} expected")
    ws = torch.empty(L.lib().p4c_grib_pack_workspace_bytes(n, T, N, K) // 4, dtype=torch.float32, device=dev)
    host_samples = (ctypes.c_int32 * n)(*samples)
    host_spec = (ctypes.c_int32 * (2 * K))(*[x for pair in spec for x in pair])
    dense = bool(L.lib().p4c_grib_pack_dense(K, F))
    per_point = 4 * F if dense else min(4 * F, 64 * K)   # whole points, or a 64-byte line per packed feature, at most the point
    L.call("p4c_grib_pack", L.ptr(p), pbs, pts, host_samples, L.ptr(std), L.ptr(mean), L.ptr(index), host_spec, int(bool(flip_rows)),
           L.ptr(params), L.ptr(packed), pitch, L.ptr(ws), B, n, T, H, W, F, K, L.stream(dev),
           alg_bytes=n * T * (N * 2 * per_point + sum((N * nbits + 7) // 8 for _, nbits in spec)))
    return params, packed


# ------------------------------------------------------------------------------------------------ GRIB2 complex packing
# launch constants of csrc/grib_pack_complex.hip (p4c_grib_pack_complex_group() / _params() / _scan_threads() report the same); its
# tiles and workgroups per launch are GRIB_TILE and GRIB_MAX_BLOCKS
GRIB_COMPLEX_GROUP = 32         # values of a group
GRIB_COMPLEX_PARAMS = 11        # int32 words of a params record: the five of grib_pack, ival1, ival2, gmin, ref_bits, length, offset
GRIB_COMPLEX_SCAN_THREADS = 256  # groups (scan), fields (offsets), 8 groups each (tables) per loop trip of a workgroup


def grib_complex_capacity(n: int, T: int, N: int, spec) -> int:
    """bytes of ``grib_pack_complex``'s ``out``: the worst case of every field, each rounded up to 4 (p4c_grib_pack_complex_capacity)"""
    from . import grib2

    return n * T * sum(grib2.complex_capacity(N, int(nbits), int(order)) for _, nbits, order in spec)


def grib_pack_complex(pred, std, mean, spec, samples=None, features=None, flip_rows=False, out=None):
    """The normalised prediction (B,T,H,W,F) -- or (B,T,N,F) -- -> GRIB2 complex packing (templates 5.2 / 5.3; p4c_grib_pack_complex):
    ``params`` (n,T,K,11) int32 -- the five words of ``grib_pack``, then ival1, ival2, gmin, ref_bits, the payload's length in octets
    and its offset -- and ``stream``, one uint8 buffer of ``grib_complex_capacity`` bytes in which field (s,t,k)'s section-7 payload
    lies at ``offset .. offset + length``; payloads follow each other in (sample, lead time, feature) order at multiples of 4, a field
    with bad > 0 has length 0, no other byte is written.  ``spec``: one (D, nbits, order) per PACKED feature, order 0 (5.2), 1 or 2
    (5.3); nbits 1 .. 32 at order 0, nbits + order <= 31 otherwise.  The integers are those of ``grib_pack``: a field decodes to the
    same fp32 plane.  The contract is in include/py4cast_hip.h and, in numpy, ``grib2.pack_complex``.  ``samples``, ``features``,
    ``flip_rows`` as in ``grib_pack``; ``out``: (params, stream) dense device tensors, stream 4-byte aligned and at least the capacity
    long.  Not differentiable."""
    L.require_cuda(pred, std, mean)
    if pred.dim() not in (4, 5):
        raise L.P4CError(f"grib_pack_complex: prediction {tuple(pred.shape)}: (B, T, H, W, F) or (B, T, N, F) expected")
    B, T, F = pred.shape[0], pred.shape[1], pred.shape[-1]
    H, W = (pred.shape[2], pred.shape[3]) if pred.dim() == 5 else (1, pred.shape[2])
    if std.numel() != F or mean.numel() != F:
        raise L.P4CError(f"grib_pack_complex: {std.numel()} standard deviations / {mean.numel()} means for {F} features")
    features = tuple(range(F)) if features is None else tuple(int(f) for f in features)
    samples = tuple(range(B)) if samples is None else tuple(int(s) for s in samples)
    if any(len(tuple(entry)) != 3 for entry in spec):
        raise L.P4CError(f"grib_pack_complex: spec {spec}: one (D, nbits, order) per packed feature expected")
    spec = [(int(D), int(nbits), int(order)) for D, nbits, order in spec]
    K, n = len(features), len(samples)
    if not 1 <= K <= GRIB_MAX_FEATURES:
        raise L.P4CError(f"grib_pack_complex: {K} features: 1 .. at most {GRIB_MAX_FEATURES} per call")
    if len(spec) != K:
        raise L.P4CError(f"grib_pack_complex: {len(spec)} (D, nbits, order) triples for {K} packed features")
    if min(features) < 0 or max(features) >= F:
        raise L.P4CError(f"grib_pack_complex: feature indices {features} leave 0 .. {F - 1}")
    if not 1 <= n <= GRIB_MAX_SAMPLES or n * T > 65535:
        raise L.P4CError(f"grib_pack_complex: {n} samples: 1 .. at most {GRIB_MAX_SAMPLES} per call, n*T <= 65535")
    if min(samples) < 0 or max(samples) >= B:
        raise L.P4CError(f"grib_pack_complex: sample indices {samples} leave 0 .. {B - 1}")
    if any(abs(D) > 15 or not 1 <= nbits <= 32 or order not in (0, 1, 2) or (order and nbits + order > 31) for D, nbits, order in spec):
        raise L.P4CError(f"grib_pack_complex: spec {spec}: |D| <= 15, an order of 0 .. 2, 1 <= nbits <= 32 at order 0 and "
                         f"nbits + order <= 31 at orders 1 and 2 expected")
    N = H * W
    capacity = grib_complex_capacity(n, T, N, spec)
    if capacity >= 2 ** 31:
        raise L.P4CError(f"grib_pack_complex: {capacity} payload bytes in the worst case: fewer than 2^31 per call")
    p, (pbs, pts) = _rows(pred.detach().float(), 2)
    dev = p.device
    std, mean = std.to(p).contiguous(), mean.to(p).contiguous()
    index = _grib_features(features, dev.index if dev.index is not None else torch.cuda.current_device())
    pshape = (n, T, K, GRIB_COMPLEX_PARAMS)
    if out is None:
        params = torch.empty(pshape, dtype=torch.int32, device=dev)
        stream = torch.empty(capacity, dtype=torch.uint8, device=dev)
    else:
        params, stream = out
        if (tuple(params.shape) != pshape or params.dtype != torch.int32 or not params.is_contiguous() or params.device != dev
                or stream.dim() != 1 or stream.numel() < capacity or stream.dtype != torch.uint8 or not stream.is_contiguous()
                or stream.device != dev or stream.data_ptr() % 4):
            raise L.P4CError(f"grib_pack_complex: out: a dense int32 {pshape} and a dense, 4-byte aligned 1-D uint8 tensor of at least "
                             f"{capacity} bytes on {dev} expected")
    ws = torch.empty((L.lib().p4c_grib_pack_complex_workspace_bytes(n, T, N, K, F) + 15) // 16 * 2, dtype=torch.int64, device=dev)
    host_samples = (ctypes.c_int32 * n)(*samples)
    host_spec = (ctypes.c_int32 * (3 * K))(*[x for triple in spec for x in triple])
    dense = bool(L.lib().p4c_grib_pack_dense(K, F))
    per_point = 4 * F if dense else min(4 * F, 64 * K)
    # dense: three reads of the prediction (range, group, pack); gather: two, and the differences (4 bytes per value) written and read;
    # the group records (16 + 4 bytes per 32 values) written and read twice; the payloads at their worst case
    ng = (N + GRIB_COMPLEX_GROUP - 1) // GRIB_COMPLEX_GROUP
    passes = N * 3 * per_point if dense else N * (2 * per_point + 8 * K)
    L.call("p4c_grib_pack_complex", L.ptr(p), pbs, pts, host_samples, L.ptr(std), L.ptr(mean), L.ptr(index), host_spec,
           int(bool(flip_rows)), L.ptr(params), L.ptr(stream), stream.numel(), L.ptr(ws), B, n, T, H, W, F, K, L.stream(dev),
           alg_bytes=n * T * (passes + K * ng * 60) + capacity)
    return params, stream


# ------------------------------------------------------------------------------------------------ GRIB2 simple packing, decoded
# launch constants of csrc/grib_unpack.hip (p4c_grib_unpack_tile() / p4c_grib_unpack_max_blocks() report the same)
GRIB_UNPACK_TILE = 2048        # points per loop trip of a workgroup, 8 per lane
GRIB_UNPACK_MAX_BLOCKS = 2048  # the most workgroups of one launch: each takes ceil(tiles / this) consecutive tiles of the call
# host mirror of p4c_grib_field (include/py4cast_hip.h)
GRIB_FIELD = np.dtype([("stream_off", "<i8"), ("stream_len", "<i8"), ("bitmap_off", "<i8"), ("dst_off", "<i8"), ("ni", "<i4"), ("nj", "<i4"),
                       ("count", "<i4"), ("nbits", "<i4"), ("E", "<i4"), ("D", "<i4"), ("R", "<f4"), ("flip_rows", "<i4"), ("tile0", "<i4"),
                       ("pad", "<i4")])


def grib_fields(records) -> np.ndarray:
    """A GRIB_FIELD table from a sequence of mappings with its column names; ``bitmap_off`` defaults to -1 (no bitmap), ``flip_rows``
    and ``dst_off`` to 0.  A GRIB_FIELD array is copied."""
    if isinstance(records, np.ndarray):
        if records.dtype != GRIB_FIELD:
            raise L.P4CError(f"grib_unpack: a table of dtype {records.dtype}, GRIB_FIELD expected")
        return records.reshape(-1).copy()
    table = np.zeros(len(records), dtype=GRIB_FIELD)
    table["bitmap_off"] = -1
    for i, rec in enumerate(records):
        for name, value in rec.items():
            if name not in GRIB_FIELD.names:
                raise L.P4CError(f"grib_unpack: field {i}: {name!r} is no column of GRIB_FIELD")
            table[i][name] = value
    return table


def grib_table(fields, dense: bool) -> np.ndarray:
    """The table ``grib_unpack`` launches with: ``grib_fields(fields)`` with ``tile0`` filled in and, with ``dense``, ``dst_off`` too:
    the planes one after the other in the order of the table, each at a multiple of 4 floats."""
    table = grib_fields(fields)
    if table.size < 1:
        raise L.P4CError("grib_unpack: no fields")
    points = table["ni"].astype(np.int64) * table["nj"].astype(np.int64)
    if points.min() < 1 or points.max() >= 2 ** 31:
        raise L.P4CError(f"grib_unpack: fields of {points.min()} .. {points.max()} points: 1 .. 2^31 - 1 expected")
    tiles = (points + GRIB_UNPACK_TILE - 1) // GRIB_UNPACK_TILE
    if int(tiles.sum()) >= 2 ** 31:
        raise L.P4CError(f"grib_unpack: {int(tiles.sum())} tiles: fewer than 2^31 per call")
    table["tile0"] = np.cumsum(tiles) - tiles
    if dense:
        padded = (points + 3) // 4 * 4
        table["dst_off"] = np.cumsum(padded) - padded
    return table


def grib_unpack(bytes_dev: torch.Tensor, fields, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The simple-packed (5.0) bit streams and bitmaps of GRIB2 fields, lying in the device byte buffer ``bytes_dev`` (uint8, dense,
    4-byte aligned) as they do in the files -> their fp32 planes in one flat device tensor (p4c_grib_unpack; the contract is in
    include/py4cast_hip.h and, in numpy, ``grib2.unpack_fields``).  ``fields``: a GRIB_FIELD array or a sequence of mappings
    (``grib_fields``); ``tile0`` is filled in here.  Without ``out`` the planes lie one after the other in the order of the table,
    each at a multiple of 4 floats (``grib_table(fields, dense=True)`` tells where); with ``out`` (flat fp32, dense) each plane goes to
    its ``dst_off`` and nothing else is written.  Returns ``out``.  The records are checked by the library, not here.  Not
    differentiable."""
    L.require_cuda(bytes_dev, out)
    if bytes_dev.dtype != torch.uint8 or bytes_dev.dim() != 1 or not bytes_dev.is_contiguous() or bytes_dev.data_ptr() % 4:
        raise L.P4CError(f"grib_unpack: bytes {tuple(bytes_dev.shape)} {bytes_dev.dtype}: a dense, 4-byte aligned 1-D uint8 tensor expected")
    table = grib_table(fields, dense=out is None)
    points = table["ni"].astype(np.int64) * table["nj"].astype(np.int64)
    total = int(((points + GRIB_UNPACK_TILE - 1) // GRIB_UNPACK_TILE).sum())
    dev = bytes_dev.device
    if out is None:
        out = torch.empty(int(((points + 3) // 4 * 4).sum()), dtype=torch.float32, device=dev)
    elif (out.dtype != torch.float32 or out.dim() != 1 or not out.is_contiguous() or out.device != dev
          or int((table["dst_off"] + points).max()) > out.numel() or int(table["dst_off"].min()) < 0):
        raise L.P4CError(f"grib_unpack: out {tuple(out.shape)} {out.dtype} on {out.device}: a dense 1-D fp32 tensor on {dev} that holds "
                         f"every plane at its dst_off expected")
    table_dev = torch.from_numpy(table.view(np.uint8)).to(dev)
    has_bitmap = bool((table["bitmap_off"] >= 0).any())
    ws = torch.empty(L.lib().p4c_grib_unpack_workspace_bytes(total) // 4, dtype=torch.int32, device=dev) if has_bitmap else None
    read = int(((table["count"].astype(np.int64) * table["nbits"] + 7) // 8).sum() + ((points + 7) // 8)[table["bitmap_off"] >= 0].sum())
    L.call("p4c_grib_unpack", L.ptr(bytes_dev), bytes_dev.numel(), L.ptr(table_dev), ctypes.c_void_p(table.ctypes.data), int(table.size),
           L.ptr(out), L.ptr(ws), L.stream(dev), alg_bytes=read + 4 * int(points.sum()))
    return out


# ------------------------------------------------------------------------------------------------ GRIB2 simple packing, windowed
GRIB_WINDOW_MAX_FEATURES = 144   # p4c_grib_window_max_features(): the LDS tile
# host mirror of p4c_grib_wfield (include/py4cast_hip.h)
GRIB_WFIELD = np.dtype([("slice_off", "<i8"), ("slice_len", "<i8"), ("bit0", "<i8"), ("bitmap_off", "<i8"), ("ni", "<i4"), ("row0", "<i4"),
                        ("row_step", "<i4"), ("col0", "<i4"), ("nbits", "<i4"), ("E", "<i4"), ("D", "<i4"), ("R", "<f4"), ("mean", "<f4"),
                        ("std", "<f4")])


def grib_wfields(records, shape=None) -> np.ndarray:
    """A GRIB_WFIELD table from a sequence of mappings with its column names; ``bitmap_off`` defaults to -1 (no bitmap), ``row_step``
    and ``std`` to 1, the rest to 0.  A GRIB_WFIELD array is copied."""
    if isinstance(records, np.ndarray):
        if records.dtype != GRIB_WFIELD:
            raise L.P4CError(f"grib_window_pack: a table of dtype {records.dtype}, GRIB_WFIELD expected")
        return np.ascontiguousarray(records).copy()
    table = np.zeros(len(records), dtype=GRIB_WFIELD)
    table["bitmap_off"], table["row_step"], table["std"] = -1, 1, 1.0
    for i, rec in enumerate(records):
        for name, value in rec.items():
            if name not in GRIB_WFIELD.names:
                raise L.P4CError(f"grib_window_pack: field {i}: {name!r} is no column of GRIB_WFIELD")
            table[i][name] = value
    return table


def grib_window_pack(bytes_dev: torch.Tensor, fields, B: int, T: int, H: int, W: int, F: int) -> torch.Tensor:
    """Windows of simple-packed GRIB2 fields without bitmap, whose slices (``grib2.window_slice``) lie in the device byte buffer
    ``bytes_dev`` (uint8, dense, 4-byte aligned) -> (B, T, H, W, F) fp32 standardised features-last, one launch of
    ``p4c_grib_window_pack`` (the contract is in include/py4cast_hip.h and, in numpy, ``grib2.unpack_window``).  ``fields``: B*T*F
    GRIB_WFIELD records (or mappings, ``grib_wfields``), element (b, t, f) at (b*T + t)*F + f.  The records are checked by the
    library, not here: a refusal raises ``P4CError`` before anything is launched.  Not differentiable."""
    L.require_cuda(bytes_dev)
    if bytes_dev.dtype != torch.uint8 or bytes_dev.dim() != 1 or not bytes_dev.is_contiguous() or bytes_dev.data_ptr() % 4:
        raise L.P4CError(f"grib_window_pack: bytes {tuple(bytes_dev.shape)} {bytes_dev.dtype}: a dense, 4-byte aligned 1-D uint8 tensor expected")
    B, T, H, W, F = int(B), int(T), int(H), int(W), int(F)
    table = grib_wfields(fields).reshape(-1)
    if min(B, T, H, W, F) < 1 or table.size != B * T * F:
        raise L.P4CError(f"grib_window_pack: {table.size} fields for B x T x F = {B} x {T} x {F} (H = {H}, W = {W})")
    if B * T * H * W >= 2 ** 31:      # the library refuses it too; here before the output is allocated
        raise L.P4CError(f"grib_window_pack: {B * T * H * W} rows: at most 2^31 - 1 per call")
    dev = bytes_dev.device
    table_dev = torch.from_numpy(table.view(np.uint8)).to(dev)
    out = torch.empty(B, T, H, W, F, dtype=torch.float32, device=dev)
    read = int((H * W * table["nbits"].astype(np.int64) + 7).sum() // 8)
    L.call("p4c_grib_window_pack", L.ptr(bytes_dev), bytes_dev.numel(), L.ptr(table_dev), ctypes.c_void_p(table.ctypes.data), L.ptr(out),
           B, T, H, W, F, L.stream(dev), alg_bytes=read + 4 * out.numel())
    return out


# ------------------------------------------------------------------------------------------------ GRIB2 complex packing, decoded
# launch constants of csrc/grib_complex.hip (p4c_grib_complex_tile() / _chunk() / _max_blocks() report the same)
GRIB_COMPLEX_TILE = 2048        # values per tile, 8 per lane
GRIB_COMPLEX_CHUNK = 1024       # groups per chunk, 4 per lane
GRIB_COMPLEX_MAX_BLOCKS = 1024  # the most workgroups of one launch
GRIB_STATUS_LENGTHS, GRIB_STATUS_WIDTH, GRIB_STATUS_STREAM = 1, 2, 4   # the bits of a field's status
# host mirror of p4c_grib_cfield (include/py4cast_hip.h)
GRIB_CFIELD = np.dtype([("stream_off", "<i8"), ("stream_len", "<i8"), ("bitmap_off", "<i8"), ("dst_off", "<i8"), ("ival1", "<i8"),
                        ("ival2", "<i8"), ("gmin", "<i8"), ("ni", "<i4"), ("nj", "<i4"), ("count", "<i4"), ("ng", "<u4"), ("ref_bits", "<i4"),
                        ("w_ref", "<i4"), ("w_bits", "<i4"), ("l_ref", "<u4"), ("l_inc", "<i4"), ("l_last", "<u4"), ("l_bits", "<i4"),
                        ("order", "<i4"), ("nbytes", "<i4"), ("E", "<i4"), ("D", "<i4"), ("R", "<f4"), ("flip_rows", "<i4"), ("tile0", "<i4"),
                        ("chunk0", "<i4"), ("pad", "<i4")])


def grib_cfields(records) -> np.ndarray:
    """A GRIB_CFIELD table from a sequence of mappings with its column names; ``bitmap_off`` defaults to -1 (no bitmap), everything
    else to 0.  A GRIB_CFIELD array is copied."""
    if isinstance(records, np.ndarray):
        if records.dtype != GRIB_CFIELD:
            raise L.P4CError(f"grib_unpack_complex: a table of dtype {records.dtype}, GRIB_CFIELD expected")
        return records.reshape(-1).copy()
    table = np.zeros(len(records), dtype=GRIB_CFIELD)
    table["bitmap_off"] = -1
    for i, rec in enumerate(records):
        for name, value in rec.items():
            if name not in GRIB_CFIELD.names:
                raise L.P4CError(f"grib_unpack_complex: field {i}: {name!r} is no column of GRIB_CFIELD")
            table[i][name] = value
    return table


def grib_ctable(fields, dense: bool) -> np.ndarray:
    """The table ``grib_unpack_complex`` launches with: ``grib_cfields(fields)`` with ``tile0`` and ``chunk0`` filled in and, with
    ``dense``, ``dst_off`` too: the planes one after the other in the order of the table, each at a multiple of 4 floats."""
    table = grib_cfields(fields)
    if table.size < 1:
        raise L.P4CError("grib_unpack_complex: no fields")
    points = table["ni"].astype(np.int64) * table["nj"].astype(np.int64)
    if points.min() < 1 or points.max() >= 2 ** 31:
        raise L.P4CError(f"grib_unpack_complex: fields of {points.min()} .. {points.max()} points: 1 .. 2^31 - 1 expected")
    tiles = (points + GRIB_COMPLEX_TILE - 1) // GRIB_COMPLEX_TILE
    chunks = np.maximum((table["ng"].astype(np.int64) + GRIB_COMPLEX_CHUNK - 1) // GRIB_COMPLEX_CHUNK, 1)
    if int(tiles.sum()) >= 2 ** 31 or int(chunks.sum()) >= 2 ** 31:
        raise L.P4CError(f"grib_unpack_complex: {int(tiles.sum())} tiles, {int(chunks.sum())} chunks: fewer than 2^31 per call")
    table["tile0"] = np.cumsum(tiles) - tiles
    table["chunk0"] = np.cumsum(chunks) - chunks
    if dense:
        padded = (points + 3) // 4 * 4
        table["dst_off"] = np.cumsum(padded) - padded
    return table


def grib_unpack_complex(bytes_dev: torch.Tensor, fields, out: Optional[torch.Tensor] = None,
                        status: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The complex-packed (5.2 / 5.3) section-7 payloads and bitmaps of GRIB2 fields, lying in the device byte buffer ``bytes_dev``
    (uint8, dense, 4-byte aligned) as they do in the files -> (their fp32 planes in one flat device tensor, one int32 status per field)
    (p4c_grib_unpack_complex; the contract is in include/py4cast_hip.h and, in numpy, ``grib2.unpack_fields``).  ``fields``: a
    GRIB_CFIELD array or a sequence of mappings (``grib_cfields``); ``tile0`` and ``chunk0`` are filled in here.  ``out`` as in
    ``grib_unpack``.  ``status`` (int32, one per field, on the device) stays there: a field whose word is not 0 (GRIB_STATUS_*: its
    stream contradicts its header) has an all-NaN plane; reading it is the caller's synchronisation.  The records are checked by the
    library, not here.  Not differentiable."""
    L.require_cuda(bytes_dev, out, status)
    if bytes_dev.dtype != torch.uint8 or bytes_dev.dim() != 1 or not bytes_dev.is_contiguous() or bytes_dev.data_ptr() % 4:
        raise L.P4CError(f"grib_unpack_complex: bytes {tuple(bytes_dev.shape)} {bytes_dev.dtype}: a dense, 4-byte aligned 1-D uint8 tensor "
                         f"expected")
    table = grib_ctable(fields, dense=out is None)
    points = table["ni"].astype(np.int64) * table["nj"].astype(np.int64)
    tiles = int(((points + GRIB_COMPLEX_TILE - 1) // GRIB_COMPLEX_TILE).sum())
    chunks = int(np.maximum((table["ng"].astype(np.int64) + GRIB_COMPLEX_CHUNK - 1) // GRIB_COMPLEX_CHUNK, 1).sum())
    dev = bytes_dev.device
    if out is None:
        out = torch.empty(int(((points + 3) // 4 * 4).sum()), dtype=torch.float32, device=dev)
    elif (out.dtype != torch.float32 or out.dim() != 1 or not out.is_contiguous() or out.device != dev
          or int((table["dst_off"] + points).max()) > out.numel() or int(table["dst_off"].min()) < 0):
        raise L.P4CError(f"grib_unpack_complex: out {tuple(out.shape)} {out.dtype} on {out.device}: a dense 1-D fp32 tensor on {dev} that "
                         f"holds every plane at its dst_off expected")
    if status is None:
        status = torch.empty(table.size, dtype=torch.int32, device=dev)
    elif status.dtype != torch.int32 or status.dim() != 1 or not status.is_contiguous() or status.device != dev or status.numel() != table.size:
        raise L.P4CError(f"grib_unpack_complex: status {tuple(status.shape)} {status.dtype} on {status.device}: {table.size} int32 on {dev} "
                         f"expected")
    table_dev = torch.from_numpy(table.view(np.uint8)).to(dev)
    has_bitmap = bool((table["bitmap_off"] >= 0).any())
    ws = torch.empty((L.lib().p4c_grib_unpack_complex_workspace_bytes(tiles, chunks, int(has_bitmap)) + 7) // 8, dtype=torch.int64, device=dev)
    read = int(table["stream_len"].sum() + ((points + 7) // 8)[table["bitmap_off"] >= 0].sum())
    L.call("p4c_grib_unpack_complex", L.ptr(bytes_dev), bytes_dev.numel(), L.ptr(table_dev), ctypes.c_void_p(table.ctypes.data),
           int(table.size), L.ptr(out), L.ptr(status), L.ptr(ws), L.stream(dev), alg_bytes=2 * read + 4 * int(points.sum()))
    return out, status
