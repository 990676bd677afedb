"""Strided convolutions of features-last bf16 maps as a patch gather (csrc/segformer.hip: p4c_seg_patch_gather, nn.Unfold's column
order c k^2 + ky k + kx, so the GEMM takes the parameter's own (D, C k^2) view) + one GEMM of csrc/gemm.hip; the data gradient is the
GEMM + the gather-form adjoint (p4c_seg_patch_scatter).

* ``patch_conv(x, w2d, b, k, stride, pad)``  gather node + ``ops_gemm.linear`` (weight / bias gradients added into ``.grad`` in place)
* ``_PatchConv``                             gather + GEMM as ONE node that leaves the batch-norm column sums of its output and returns
  its weight gradient to autograd

No CPU fallback: every entry point raises on CPU tensors."""

from typing import Optional

import torch

from . import _lib as L
from . import ops_gemm as G


def _gather_fwd(x: torch.Tensor, k: int, stride: int, pad: int):
    """(cols (B, Ho, Wo, C k^2), geom) = nn.Unfold(k, stride, pad) of a features-last map; geom is what _scatter_bwd needs"""
    xc = x.contiguous()
    B, H, W, C = xc.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cols = torch.empty(B, Ho, Wo, C * k * k, dtype=xc.dtype, device=xc.device)
    L.call("p4c_seg_patch_gather", L.ptr(xc), L.ptr(cols), B, H, W, C, k, stride, pad, L.stream(xc.device),
           alg_bytes=2 * (xc.numel() + cols.numel()))
    return cols, (B, H, W, C, k, stride, pad)


def _scatter_bwd(dcols: torch.Tensor, geom) -> torch.Tensor:
    """dx (B, H, W, C): the adjoint of _gather_fwd"""
    B, H, W, C, k, stride, pad = geom
    dcols = dcols.contiguous()
    dx = torch.empty(B, H, W, C, dtype=dcols.dtype, device=dcols.device)
    L.call("p4c_seg_patch_scatter", L.ptr(dcols), L.ptr(dx), B, H, W, C, k, stride, pad, C, L.stream(dcols.device),
           alg_bytes=2 * (dx.numel() + dcols.numel()))
    return dx


class _PatchGather(torch.autograd.Function):
    """cols (B, Ho, Wo, C k^2) = nn.Unfold(k, stride, pad) of a features-last map, columns in Unfold's order c k^2 + ky k + kx"""

    @staticmethod
    def forward(ctx, x, k, stride, pad):
        cols, ctx.geom = _gather_fwd(x, k, stride, pad)
        return cols

    @staticmethod
    def backward(ctx, dcols):
        return _scatter_bwd(dcols, ctx.geom), None, None, None


def patch_conv(x: torch.Tensor, w2d: torch.Tensor, b: Optional[torch.Tensor], k: int, stride: int, pad: int) -> torch.Tensor:
    """Conv2d(C, D, k, stride, pad) of a features-last bf16 map with the weight given as its (D, C k^2) view (Unfold's column order)"""
    L.require_cuda(x)
    if x.dtype != torch.bfloat16 or x.dim() != 4 or w2d.shape[1] != x.shape[-1] * k * k:
        raise L.P4CError(f"ops_patch.patch_conv: unsupported operands (x {tuple(x.shape)} {x.dtype}, w {tuple(w2d.shape)}, k {k})")
    if k == 1 and stride == 1 and pad == 0:
        return G.linear(x, w2d, b)
    return G.linear(_PatchGather.apply(x, k, stride, pad), w2d, b)


class _PatchConv(torch.autograd.Function):
    """y (B, Ho, Wo, Co) = Conv2d(C, Co, k, stride, pad, bias=False) of a features-last bf16 map as a patch gather + one GEMM whose
    epilogue leaves the batch-norm column sums; w2d = the weight's (Co, C k^2) view"""

    @staticmethod
    def forward(ctx, x, w2d, k, stride, pad):
        cols, ctx.geom = _gather_fwd(x, k, stride, pad)
        B, Ho, Wo, K = cols.shape
        Co = w2d.shape[0]
        c2 = cols.view(-1, K)
        fwd, dgr = G.weight_images(w2d, 1)
        y, _, stats = G.gemm_nt(c2, fwd, Co, K, want_stats=True)
        ctx.save_for_backward(c2, dgr)
        ctx.pgeom, ctx.wdtype = (B, Ho, Wo, K, Co), w2d.dtype
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return y.view(B, Ho, Wo, Co), stats

    @staticmethod
    def backward(ctx, dy, _dstats):
        c2, dgr = ctx.saved_tensors
        B, Ho, Wo, K, Co = ctx.pgeom
        dy2 = G._rows(dy, Co)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _scatter_bwd(G.gemm_nt(dy2, dgr, K, Co)[0].view(B, Ho, Wo, K), ctx.geom)
        dw = None
        if ctx.needs_input_grad[1]:
            dw, _ = G.gemm_tn(dy2, c2, Co, K)
            dw = dw.to(ctx.wdtype)
        return dx, dw, None, None, None
