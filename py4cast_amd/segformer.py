"""
Segformer on MI355X -- the model behind ``model_name: Segformer`` (the reference's config/CLI/model/segformer.yaml; registry key
``Segformer`` of its tests/test_models.py).  The reference takes the class from mfai v5.0.1, which wraps lucidrains' segformer-pytorch
and is absent here: PARITY UNPINNED; the network is restated in tests/segformer_reference.py (float64) and checked against that.

The network, on features-last maps (B, H, W, C); state-dict keys are mfai's:
* ``downsampler`` = Conv2d(in, num_downsampling_chans, 3, stride 2, padding 1);
* ``mit.stages.{s}`` = (nn.Unfold(k, stride, pad), Conv2d(C_in k^2, dims[s], 1), layers) with (k, stride, pad) = (7, 4, 3), then
  (3, 2, 1) three times; each of the ``num_layers`` layers is x = attn(norm(x)) + x; x = ff(norm(x)) + x (PreNorm);
* the norm is lucidrains' LayerNorm over the channels: (x - mean) / (sqrt(var_biased) + 1e-5) g + b -- eps on the standard deviation;
* attn = EfficientSelfAttention: to_q (1x1), to_kv (r x r, stride r), to_out (1x1), all without bias; per head (head_dim = dims / heads)
  softmax(q k^T head_dim^-1/2) v with the keys / values of the r x r-reduced map;
* ff = MixFeedForward: Conv2d(d, h, 1) -> DsConv2d (depthwise 3x3 with bias -> Conv2d(h, h, 1)) -> GELU (erf) -> Conv2d(h, d, 1);
* decoder: to_fused[i] = Conv2d(dims[i], decoder_dim, 1) + nearest up-sampling by 2^i, cat, to_segmentation = Conv2d(4 decoder_dim,
  decoder_dim, 1) -> Conv2d(decoder_dim, out, 1), then bilinear up-sampling by 8 (align_corners = False) to the input grid.
Assumptions of the restatement (mfai's own call is not on this machine): the final bilinear mode with align_corners = False, and the
LayerNorm form above.

What runs where, bf16 (``compute_dtype`` / ``activation_dtype`` "bf16"):
* every 1x1 convolution: the GEMMs of csrc/gemm.hip (``ops_gemm.linear`` / ``ops_gemm.mlp``: the pointwise half of DsConv2d, GELU and
  the second FFN convolution are ONE node, GELU in the epilogue, GELU' in the data gradient's epilogue); the residual adds: forward in
  the epilogues of to_out / fc2, backward inside the LayerNorm's backward launch (the residual takes x from the norm's passthrough);
* the strided convolutions (downsampler, patch embeddings, the key / value reduction): ``ops_patch.patch_conv``, a patch gather
  (csrc/segformer.hip) in nn.Unfold's column order, so the GEMM takes the parameter's own (D, C k^2) view; data gradient: the gather-form adjoint;
* LayerNorm, the depthwise 3x3 convolution, the spatial-reduction attention core and the decoder's nearest up-sampling sum: csrc/segformer.hip;
* the decoder applies to_segmentation.0 per stage at the stage's resolution (its column block of the weight) and sums the nearest
  up-sampled results -- the same linear map as up-sampling, concatenating and convolving, without the 4 x decoder_dim buffer;
* the final bilinear x8: csrc/resize.hip on the head's output padded to a multiple of 8 channels.
fp32 (the parity flavour): the same network on the library, NCHW inside.
"""

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from . import ops_gemm as G
from .base import ModelType
from .conv_model import ConvModelMI355X, cast_out, crop_channels, pad_head, pad_rows, pad_weight_in
from .ops_patch import patch_conv

try:
    from dataclasses_json import dataclass_json
except Exception:  # pragma: no cover
    def dataclass_json(cls):
        return cls

STAGE_KSP = ((7, 4, 3), (3, 2, 1), (3, 2, 1), (3, 2, 1))     # (kernel, stride, padding) of the four patch embeddings
NATIVE_HEAD_DIM = 32
NATIVE_MAX_KEYS = 256


@dataclass_json
@dataclass
class SegformerSettings:
    """mfai's SegformerSettings fields (config/CLI/model/segformer.yaml) + the MI355X knobs."""

    dims: Tuple[int, ...] = (32, 64, 160, 256)
    heads: Tuple[int, ...] = (1, 2, 5, 8)
    ff_expansion: Tuple[int, ...] = (8, 8, 4, 4)
    reduction_ratio: Tuple[int, ...] = (8, 4, 2, 1)
    num_layers: int = 2
    decoder_dim: int = 256
    num_downsampling_chans: int = 32
    # MI355X-specific
    compute_dtype: str = "f32"      # "f32" (library operations, the parity flavour) or "bf16" (the native route)
    activation_dtype: Optional[str] = None   # HBM storage of activations: "f32" | "bf16"; None = compute_dtype


# ---------------------------------------------------------------- the modules (mfai's / lucidrains' names; NCHW forward = fp32 route)
class ChanLayerNorm(nn.Module):
    """lucidrains' LayerNorm over the channels of an NCHW map: (x - mean) / (std + eps) * g + b"""

    def __init__(self, dim: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.g = nn.Parameter(torch.ones(1, dim, 1, 1))
        self.b = nn.Parameter(torch.zeros(1, dim, 1, 1))

    def forward(self, x):
        std = torch.var(x, dim=1, unbiased=False, keepdim=True).sqrt()
        mean = torch.mean(x, dim=1, keepdim=True)
        return (x - mean) / (std + self.eps) * self.g + self.b


class PreNorm(nn.Module):
    def __init__(self, dim: int, fn: nn.Module):
        super().__init__()
        self.fn = fn
        self.norm = ChanLayerNorm(dim)

    def forward(self, x):
        return self.fn(self.norm(x))


class DsConv2d(nn.Module):
    def __init__(self, dim_in: int, dim_out: int, kernel_size: int, padding: int, stride: int = 1, bias: bool = True):
        super().__init__()
        self.net = nn.Sequential(
            nn.Conv2d(dim_in, dim_in, kernel_size=kernel_size, padding=padding, groups=dim_in, stride=stride, bias=bias),
            nn.Conv2d(dim_in, dim_out, kernel_size=1, bias=bias),
        )

    def forward(self, x):
        return self.net(x)


class EfficientSelfAttention(nn.Module):
    def __init__(self, dim: int, heads: int, reduction_ratio: int):
        super().__init__()
        self.scale = (dim // heads) ** -0.5
        self.heads = heads
        self.reduction_ratio = reduction_ratio
        self.to_q = nn.Conv2d(dim, dim, 1, bias=False)
        self.to_kv = nn.Conv2d(dim, dim * 2, reduction_ratio, stride=reduction_ratio, bias=False)
        self.to_out = nn.Conv2d(dim, dim, 1, bias=False)

    def forward(self, x):
        B, D, h, w = x.shape
        nh = self.heads
        q = self.to_q(x)
        k, v = self.to_kv(x).chunk(2, dim=1)
        q, k, v = (t.reshape(B * nh, D // nh, -1).transpose(1, 2) for t in (q, k, v))
        attn = (q @ k.transpose(1, 2) * self.scale).softmax(dim=-1)
        out = (attn @ v).transpose(1, 2).reshape(B, D, h, w)
        return self.to_out(out)


class MixFeedForward(nn.Module):
    def __init__(self, dim: int, expansion_factor: int):
        super().__init__()
        hidden = dim * expansion_factor
        self.net = nn.Sequential(nn.Conv2d(dim, hidden, 1), DsConv2d(hidden, hidden, 3, padding=1), nn.GELU(), nn.Conv2d(hidden, dim, 1))

    def forward(self, x):
        return self.net(x)


class MiT(nn.Module):
    def __init__(self, channels: int, dims, heads, ff_expansion, reduction_ratio, num_layers: int):
        super().__init__()
        dims_all = (channels, *dims)
        self.stages = nn.ModuleList([])
        for (din, dout), (k, s, p), nh, ff, r in zip(zip(dims_all[:-1], dims_all[1:]), STAGE_KSP, heads, ff_expansion, reduction_ratio):
            layers = nn.ModuleList([nn.ModuleList([PreNorm(dout, EfficientSelfAttention(dout, nh, r)),
                                                   PreNorm(dout, MixFeedForward(dout, ff))]) for _ in range(num_layers)])
            self.stages.append(nn.ModuleList([nn.Unfold(k, stride=s, padding=p), nn.Conv2d(din * k * k, dout, 1), layers]))

    def forward(self, x):
        outs = []
        for (k, s, p), (unfold, embed, layers) in zip(STAGE_KSP, self.stages):
            B, _, h, w = x.shape
            ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
            x = embed(unfold(x).reshape(B, -1, ho, wo))
            for attn, ff in layers:
                x = attn(x) + x
                x = ff(x) + x
            outs.append(x)
        return outs


# ---------------------------------------------------------------- native nodes (bf16 rows, fp32 parameters)
def _grad_sinks(*params):
    """views of the parameters' .grad buffers (ops_gemm._sink's rule), or None when any is missing: then autograd gets the gradients"""
    if not (G.GRADS_IN_PLACE and all(p is not None and p.requires_grad for p in params)):
        return None
    from .ops_rows import grad_view

    views = [grad_view(p) for p in params]
    if any(v is None or v is False or not v.is_contiguous() for v in views):
        return None
    return views


def _reduce_into(partial, nb, outs, sinks, dev):
    """the fixed-order sum of a [nb][n1 + n2] partial table into two fp32 results: ADDED into the .grad views `sinks` (and reported to
    the gradient exchange), or written into fresh tensors of the shapes `outs` that are returned"""
    n1, n2 = outs[0].numel(), outs[1].numel()
    if sinks is not None:
        L.call("p4c_seg_reduce_partials", L.ptr(partial), nb, n1, L.ptr(sinks[0]), n2, L.ptr(sinks[1]), 1, L.stream(dev))
        L.grad_written(*sinks)
        return None, None
    o1 = torch.empty(outs[0].shape, dtype=torch.float32, device=dev)
    o2 = torch.empty(outs[1].shape, dtype=torch.float32, device=dev)
    L.call("p4c_seg_reduce_partials", L.ptr(partial), nb, n1, L.ptr(o1), n2, L.ptr(o2), 0, L.stream(dev))
    return o1, o2


class _ChanLayerNorm(torch.autograd.Function):
    """y = chan_ln(x); with passthrough, x itself is a second output: the block's residual connection takes x from there, so its
    gradient arrives here and is added inside the backward launch (no separate add of the two gradients of x)"""

    @staticmethod
    def forward(ctx, x, g, b, eps, passthrough):
        xc = x.contiguous()
        C = xc.shape[-1]
        R = xc.numel() // C
        dev = xc.device
        y = torch.empty_like(xc)
        stats = torch.empty(R, 2, dtype=torch.float32, device=dev)
        g32 = G._f32(g).reshape(C)
        L.call("p4c_seg_chan_ln_fwd", L.ptr(xc), L.ptr(g32), L.ptr(G._f32(b).reshape(C)), float(eps), L.ptr(y), L.ptr(stats), R, C, L.stream(dev),
               alg_bytes=2 * 2 * xc.numel())
        ctx.save_for_backward(xc, stats, g32)
        ctx.eps, ctx.pshape = float(eps), g.shape
        ctx.sinks = _grad_sinks(g, b)
        ctx.set_materialize_grads(False)
        return y, (x if passthrough else None)

    @staticmethod
    def backward(ctx, dy, dpass):
        xc, stats, g32 = ctx.saved_tensors
        C = xc.shape[-1]
        R = xc.numel() // C
        dev = xc.device
        if dy is None:
            return dpass, None, None, None, None
        dy = dy.contiguous()
        dadd = None
        if dpass is not None:
            dadd = dpass.contiguous() if dpass.dtype == xc.dtype else dpass.to(xc.dtype).contiguous()
        nb = L.lib().p4c_seg_chan_ln_bwd_blocks(R)
        partial = torch.empty(nb, 2, C, dtype=torch.float32, device=dev)
        dx = torch.empty_like(xc)
        L.call("p4c_seg_chan_ln_bwd", L.ptr(xc), L.ptr(dy), L.ptr(g32), L.ptr(stats), ctx.eps, L.ptr(dadd), L.ptr(dx), L.ptr(partial), R, C,
               L.stream(dev), alg_bytes=2 * (3 + (dadd is not None)) * xc.numel())
        like = torch.empty(0)
        dg, db = _reduce_into(partial, nb, (like.new_empty(ctx.pshape), like.new_empty(ctx.pshape)), ctx.sinks, dev)
        return dx, dg, db, None, None


def chan_layer_norm(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float = 1e-5, passthrough: bool = False):
    """lucidrains' channel LayerNorm (eps on the standard deviation) of features-last bf16 rows (C up to 512), fp32 g / b.
    ``passthrough``: returns (y, x') -- hand x' to x's other consumer (the residual connection) and its gradient is added inside this
    node's backward launch"""
    L.require_cuda(x)
    if x.dtype != torch.bfloat16 or x.shape[-1] > 512 or g.numel() != x.shape[-1] or b.numel() != x.shape[-1]:
        raise L.P4CError(f"segformer.chan_layer_norm: unsupported operands (x {tuple(x.shape)} {x.dtype}, g {tuple(g.shape)})")
    y, xp = _ChanLayerNorm.apply(x, g, b, float(eps), bool(passthrough))
    return (y, xp) if passthrough else y


class _Depthwise3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        xc = x.contiguous()
        B, H, W, C = xc.shape
        dev = xc.device
        w32 = G._f32(w).reshape(C, 9)
        y = torch.empty_like(xc)
        L.call("p4c_seg_dw3x3_fwd", L.ptr(xc), L.ptr(w32), L.ptr(G._f32(b)), L.ptr(y), B, H, W, C, L.stream(dev), alg_bytes=2 * 2 * xc.numel())
        ctx.save_for_backward(xc, w32)
        ctx.shapes = (w.shape, None if b is None else b.shape)
        ctx.sinks = _grad_sinks(w, b) if b is not None else None
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, w32 = ctx.saved_tensors
        B, H, W, C = xc.shape
        dev = xc.device
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(xc)
            L.call("p4c_seg_dw3x3_dgrad", L.ptr(dy), L.ptr(w32), L.ptr(dx), B, H, W, C, L.stream(dev), alg_bytes=2 * 2 * xc.numel())
        dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            rows = L.lib().p4c_seg_dw3x3_wgrad_rows(B, H, W)
            partial = torch.empty(rows, 10 * C, dtype=torch.float32, device=dev)
            L.call("p4c_seg_dw3x3_wgrad", L.ptr(xc), L.ptr(dy), L.ptr(partial), B, H, W, C, L.stream(dev), alg_bytes=2 * 2 * xc.numel())
            wshape, bshape = ctx.shapes
            like = torch.empty(0)
            dw, db = _reduce_into(partial, rows, (like.new_empty(wshape), like.new_empty(bshape if bshape is not None else (C,))), ctx.sinks, dev)
            if bshape is None:
                db = None
        return dx, dw, db


def depthwise3x3(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    """Conv2d(C, C, 3, padding=1, groups=C) (+ bias) of a features-last bf16 map, C a multiple of 8, fp32 (C, 1, 3, 3) weight"""
    L.require_cuda(x)
    C = x.shape[-1]
    if x.dtype != torch.bfloat16 or x.dim() != 4 or C % 8 or tuple(w.shape) != (C, 1, 3, 3):
        raise L.P4CError(f"segformer.depthwise3x3: unsupported operands (x {tuple(x.shape)} {x.dtype}, w {tuple(w.shape)})")
    return _Depthwise3x3.apply(x, w, b)


class _SRAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, kv, heads, scale):
        qc, kvc = q.contiguous(), kv.contiguous()
        B, Nq, D = qc.shape
        Nk = kvc.shape[1]
        dev = qc.device
        out = torch.empty_like(qc)
        lse = torch.empty(B, heads, Nq, dtype=torch.float32, device=dev)
        L.call("p4c_seg_sra_fwd", L.ptr(qc), L.ptr(kvc), L.ptr(out), L.ptr(lse), B, Nq, Nk, heads, float(scale), L.stream(dev),
               alg_bytes=2 * (2 * qc.numel() + kvc.numel()), alg_flops=4 * B * Nq * Nk * D)
        ctx.save_for_backward(qc, kvc, out, lse)
        ctx.heads, ctx.scale = heads, float(scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qc, kvc, out, lse = ctx.saved_tensors
        B, Nq, D = qc.shape
        Nk = kvc.shape[1]
        dev = qc.device
        dout = dout.contiguous()
        dq = torch.empty_like(qc)
        dkv = torch.empty_like(kvc)
        nbytes = L.lib().p4c_seg_sra_bwd_workspace_bytes(B, Nq, Nk, ctx.heads)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        L.call("p4c_seg_sra_bwd", L.ptr(qc), L.ptr(kvc), L.ptr(out), L.ptr(dout), L.ptr(lse), L.ptr(dq), L.ptr(dkv), L.ptr(ws), B, Nq, Nk,
               ctx.heads, ctx.scale, L.stream(dev), alg_bytes=2 * (4 * qc.numel() + 2 * kvc.numel()), alg_flops=8 * B * Nq * Nk * D)
        return dq, dkv, None, None


def sr_attention(q: torch.Tensor, kv: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """per head h: softmax(q_h k_h^T scale) v_h for q (B, Nq, heads 32) and kv (B, Nk, 2 heads 32) bf16 rows (k: the first heads 32
    columns, v: the rest), Nk up to 256; returns (B, Nq, heads 32) rows"""
    L.require_cuda(q)
    B, Nq, D = q.shape
    if (q.dtype != torch.bfloat16 or kv.dtype != torch.bfloat16 or D != heads * NATIVE_HEAD_DIM or kv.dim() != 3 or kv.shape[0] != B
            or kv.shape[2] != 2 * D or not (1 <= kv.shape[1] <= NATIVE_MAX_KEYS)):
        raise L.P4CError(f"segformer.sr_attention: unsupported operands (q {tuple(q.shape)}, kv {tuple(kv.shape)}, heads {heads})")
    return _SRAttention.apply(q, kv, int(heads), float(scale))


class _UpSum(torch.autograd.Function):
    """out (B, H, W, C) = z0 + sum_l nearest_up_{2^l}(z_l), l = 1..3"""

    @staticmethod
    def forward(ctx, z0, z1, z2, z3):
        zs = [z.contiguous() for z in (z0, z1, z2, z3)]
        B, H, W, C = zs[0].shape
        out = torch.empty_like(zs[0])
        L.call("p4c_seg_upsum_fwd", *[L.ptr(z) for z in zs], L.ptr(out), B, H, W, C, L.stream(out.device),
               alg_bytes=2 * (sum(z.numel() for z in zs) + out.numel()))
        ctx.geom = (B, H, W, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, H, W, C = ctx.geom
        dout = dout.contiguous()
        dz = [torch.empty(B, H >> lv, W >> lv, C, dtype=dout.dtype, device=dout.device) for lv in (1, 2, 3)]
        L.call("p4c_seg_upsum_bwd", L.ptr(dout), *[L.ptr(d) for d in dz], B, H, W, C, L.stream(dout.device),
               alg_bytes=2 * (dout.numel() * 3 + sum(d.numel() for d in dz)))
        return (dout, *dz)


def up_sum(z0, z1, z2, z3) -> torch.Tensor:
    """z0 + nearest x2 (z1) + nearest x4 (z2) + nearest x8 (z3) of features-last bf16 maps (z_l (B, H / 2^l, W / 2^l, C), C % 8 == 0)"""
    L.require_cuda(z0)
    B, H, W, C = z0.shape
    for lv, z in enumerate((z1, z2, z3), start=1):
        if z.dtype != torch.bfloat16 or tuple(z.shape) != (B, H >> lv, W >> lv, C):
            raise L.P4CError(f"segformer.up_sum: level {lv} map {tuple(z.shape)} does not match {tuple(z0.shape)}")
    if z0.dtype != torch.bfloat16 or C % 8 or H % 8 or W % 8:
        raise L.P4CError(f"segformer.up_sum: unsupported map {tuple(z0.shape)} {z0.dtype}")
    return _UpSum.apply(z0, z1, z2, z3)


# ---------------------------------------------------------------- the model
class SegformerMI355X(ConvModelMI355X):
    """mfai's Segformer (module docstring) on the native kernels of this package."""

    settings_kls = SegformerSettings
    model_type = ModelType.VISION_TRANSFORMER

    def __init__(self, in_channels: int, out_channels: int, input_shape: tuple = None, settings: SegformerSettings = SegformerSettings(),
                 *args, **kwargs):
        super().__init__(in_channels, out_channels, input_shape, settings)
        s = settings
        self._resolve_dtypes(s)
        dims, heads, ffx, rr = tuple(s.dims), tuple(s.heads), tuple(s.ff_expansion), tuple(s.reduction_ratio)
        if not (len(dims) == len(heads) == len(ffx) == len(rr) == 4):
            raise ValueError("SegformerMI355X: dims, heads, ff_expansion and reduction_ratio need four entries (four stages)")
        if any(d % h for d, h in zip(dims, heads)):
            raise ValueError(f"SegformerMI355X: every dim must be divisible by its head count, got dims {dims} heads {heads}")
        if self.native:
            if any(d // h != NATIVE_HEAD_DIM for d, h in zip(dims, heads)):
                raise ValueError(f"SegformerMI355X: the bf16 route serves head_dim {NATIVE_HEAD_DIM} only, got dims {dims} heads {heads}")
            hidden = [d * f for d, f in zip(dims, ffx)]
            if any(c % 8 for c in (*dims, *hidden, s.decoder_dim, s.num_downsampling_chans)):
                raise ValueError("SegformerMI355X: the bf16 route needs every channel count (dims, FFN widths, decoder_dim, "
                                 "num_downsampling_chans) divisible by 8")
            if max(dims) > 512:
                raise ValueError("SegformerMI355X: the bf16 route's LayerNorm serves dims up to 512")
        self.dims, self.heads, self.ratios = dims, heads, rr
        if input_shape is not None:
            self.check_grid(int(input_shape[0]), int(input_shape[1]))
        self.downsampler = nn.Conv2d(in_channels, s.num_downsampling_chans, 3, stride=2, padding=1)
        self.mit = MiT(s.num_downsampling_chans, dims, heads, ffx, rr, s.num_layers)
        self.to_fused = nn.ModuleList([nn.Sequential(nn.Conv2d(d, s.decoder_dim, 1), nn.Upsample(scale_factor=2 ** i))
                                       for i, d in enumerate(dims)])
        self.to_segmentation = nn.Sequential(nn.Conv2d(4 * s.decoder_dim, s.decoder_dim, 1), nn.Conv2d(s.decoder_dim, out_channels, 1))
        self.timed_entry_points = ("p4c_gemm_nt", "p4c_gemm_tn", "p4c_seg_patch_gather", "p4c_seg_patch_scatter", "p4c_seg_chan_ln_fwd",
                                   "p4c_seg_chan_ln_bwd", "p4c_seg_dw3x3_fwd", "p4c_seg_dw3x3_dgrad", "p4c_seg_dw3x3_wgrad", "p4c_seg_sra_fwd",
                                   "p4c_seg_sra_bwd", "p4c_seg_upsum_fwd", "p4c_seg_upsum_bwd")
        self.prefers_hip_graph = True            # ~10^3 small launches per training step: replayed from a HIP graph (profiles/segformer_*)
        self.check_required_attributes()

    def check_grid(self, H: int, W: int) -> None:
        """raise ValueError unless every stride and every r x r key reduction divides the (H, W) grid exactly (multiples of 64 with
        the default settings) and, on the bf16 route, every stage keeps at most 256 keys"""
        if H % 64 or W % 64:
            raise ValueError(f"SegformerMI355X: the grid {H}x{W} must be a multiple of 64 in both dimensions")
        for s, r in enumerate(self.ratios):
            hs, ws = H // (8 << s), W // (8 << s)
            if hs % r or ws % r:
                raise ValueError(f"SegformerMI355X: stage {s + 1} map {hs}x{ws} is not divisible by its reduction ratio {r}")
            if self.native and (hs // r) * (ws // r) > NATIVE_MAX_KEYS:
                raise ValueError(f"SegformerMI355X: the bf16 route serves up to {NATIVE_MAX_KEYS} keys per stage; the grid {H}x{W} gives "
                                 f"{(hs // r) * (ws // r)} at stage {s + 1}")

    # ---------------------------------------------------------------- fp32: the library
    def _forward_library(self, x: torch.Tensor) -> torch.Tensor:
        x = x[..., : self.in_channels].permute(0, 3, 1, 2)
        x = self.downsampler(x)
        outs = self.mit(x)
        fused = torch.cat([tf(o) for o, tf in zip(outs, self.to_fused)], dim=1)
        y = self.to_segmentation(fused)
        y = F.interpolate(y, scale_factor=8, mode="bilinear", align_corners=False)
        return y.permute(0, 2, 3, 1)

    # ---------------------------------------------------------------- bf16: the native route
    def _attn(self, pn: PreNorm, x: torch.Tensor) -> torch.Tensor:
        a = pn.fn
        B, h, w, D = x.shape
        r = a.reduction_ratio
        xn, xr = chan_layer_norm(x, pn.norm.g, pn.norm.b, pn.norm.eps, passthrough=True)
        q = G.linear(xn, a.to_q.weight.view(D, D))
        kv = patch_conv(xn, a.to_kv.weight.view(2 * D, D * r * r), None, r, r, 0)
        o = sr_attention(q.view(B, h * w, D), kv.view(B, -1, 2 * D), a.heads, a.scale)
        return G.linear(o.view(B, h, w, D), a.to_out.weight.view(D, D), res=xr)

    def _ff(self, pn: PreNorm, x: torch.Tensor) -> torch.Tensor:
        fc1, ds, _, fc2 = pn.fn.net
        dw, pw = ds.net
        D, Hd = x.shape[-1], fc1.out_channels
        xn, xr = chan_layer_norm(x, pn.norm.g, pn.norm.b, pn.norm.eps, passthrough=True)
        h1 = G.linear(xn, fc1.weight.view(Hd, D), fc1.bias)
        h2 = depthwise3x3(h1, dw.weight, dw.bias)
        return G.mlp(h2, pw.weight.view(Hd, Hd), pw.bias, fc2.weight.view(D, Hd), fc2.bias, res=xr)

    def _forward_native(self, x: torch.Tensor) -> torch.Tensor:
        x = pad_rows(x, self.cin_pad).contiguous()
        wd = pad_weight_in(self.downsampler.weight, x.shape[-1])
        x = patch_conv(x, wd.reshape(wd.shape[0], -1), self.downsampler.bias, 3, 2, 1)
        feats = []
        for (k, st, p), (_, embed, layers) in zip(STAGE_KSP, self.mit.stages):
            x = patch_conv(x, embed.weight.view(embed.out_channels, -1), embed.bias, k, st, p)
            for attn, ff in layers:
                x = self._attn(attn, x)
                x = self._ff(ff, x)
            feats.append(x)
        seg0, seg1 = self.to_segmentation
        dd = seg0.out_channels
        w0 = seg0.weight.view(dd, -1)
        zs = []
        for i, (f, tf) in enumerate(zip(feats, self.to_fused)):
            conv = tf[0]
            fi = G.linear(f, conv.weight.view(dd, -1), conv.bias)
            zs.append(G.linear(fi, w0[:, i * dd: (i + 1) * dd], seg0.bias if i == 0 else None))
        y = up_sum(*zs)
        O = seg1.out_channels
        w1, b1 = pad_head(seg1.weight.view(O, dd), seg1.bias)      # (8-channel granularity: sliced off after the up-sampling)
        return crop_channels(G.upsample_add(G.linear(y, w1, b1), None, 8), O)

    # ---------------------------------------------------------------- nn.Module API
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, H, W, in_channels) (or the rollout's zero-padded rows) -> (B, H, W, out_channels).  The fp32 route (library
        operations only) also runs on the host."""
        if self.native:
            L.require_cuda(x)
        H, W = x.shape[1], x.shape[2]
        try:
            self.check_grid(H, W)
        except ValueError as e:
            raise L.P4CError(str(e)) from None
        if x.shape[-1] < self.in_channels:
            raise L.P4CError(f"SegformerMI355X: expected {self.in_channels} input channels, got {x.shape[-1]}")
        out_dtype = x.dtype
        x = x.to(self.act_dtype)
        y = self._forward_native(x) if self.native else self._forward_library(x)
        return cast_out(y, out_dtype)
