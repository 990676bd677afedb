"""Autograd nodes of the bf16 route of HalfUNet with Ghost blocks (csrc/ghost.hip; include/py4cast_hip.h: p4c_ghost_tail_*,
p4c_halfunet_merge_*) and the encoder tail on dense maps (csrc/unet.hip: p4c_unet_enc_tail_* with ld = C):

* ``ghost_tail(prim, w)``          (z, stats): z (B,H,W,64) = [prim | depthwise3x3(prim; w)] and the batch norm's column sums of z as stored
* ``halfunet_merge(a0, .., a4)``   a0 + sum_k bilinear_up_{2^k}(a_k), one write; the adjoint of the four up-samplings from one read of dS
* ``bn_relu_pool(z, stats, bn)``   (relu(bn(z)), max_pool2d(relu(bn(z)), 2)) in one pass each way

Features-last maps, fp32 or bf16 storage, fp32 sums.  No host synchronisation, no CPU fallback."""

import torch

from . import _lib as L
from . import ops_gemm as G


def _check_map(name, t, C):
    if t.dim() != 4 or t.shape[-1] != C or t.dtype not in (torch.float32, torch.bfloat16):
        raise L.P4CError(f"{name}: a (B,H,W,{C}) fp32 or bf16 map expected, got {tuple(t.shape)} {t.dtype}")


class _GhostTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prim, w, want_stats):
        B, H, W, _ = prim.shape
        pc = prim.contiguous()
        wf = w.detach().float().reshape(32, 9).contiguous()
        es = pc.element_size()
        z = torch.empty(B, H, W, 64, dtype=pc.dtype, device=pc.device)
        stats = None
        if want_stats:
            stats = torch.empty(L.lib().p4c_ghost_tail_blocks(B, H, W), 2, 64, dtype=torch.float32, device=pc.device)
        L.call("p4c_ghost_tail_fwd", L.ptr(pc), 32, L.ptr(wf), L.ptr(z), 64, L.ptr(stats), L.dtype_code(pc.dtype), B, H, W, L.stream(pc.device),
               alg_bytes=es * B * H * W * (32 + 64))
        ctx.save_for_backward(pc, wf)
        ctx.wdtype, ctx.wshape = w.dtype, w.shape
        ctx.sink = G._sink(w, None)
        ctx.set_materialize_grads(False)
        if want_stats:
            ctx.mark_non_differentiable(stats)
        return z, stats

    @staticmethod
    def backward(ctx, dz, _dstats):
        if dz is None:
            return None, None, None
        pc, wf = ctx.saved_tensors
        B, H, W, _ = pc.shape
        dz = dz.contiguous()
        es = pc.element_size()
        dprim = torch.empty_like(pc)
        wpart = torch.empty(L.lib().p4c_ghost_tail_bwd_blocks(B, H, W), 32, 9, dtype=torch.float32, device=pc.device)
        L.call("p4c_ghost_tail_bwd", L.ptr(dz), L.ptr(pc), 32, L.ptr(wf), L.ptr(dprim), 32, L.ptr(wpart), L.dtype_code(pc.dtype), B, H, W,
               L.stream(pc.device), alg_bytes=es * B * H * W * (64 + 32 + 32))
        dw = None
        if ctx.needs_input_grad[1]:
            dw = wpart.sum(dim=0).view(ctx.wshape)          # the workgroups' partials, in their order
            if ctx.sink is not None:
                gw = ctx.sink[0]
                gw.add_(dw)
                L.grad_written(gw)
                dw = None
            else:
                dw = dw.to(ctx.wdtype)
        return (dprim if ctx.needs_input_grad[0] else None), dw, None


def ghost_tail(prim: torch.Tensor, w: torch.Tensor, want_stats: bool = True):
    """prim (B,H,W,32), the primary convolution's output; w (32,1,3,3), the depthwise "cheap operation" -> (z, stats): z (B,H,W,64) =
    [prim | depthwise3x3(prim)], stats (blocks, 2, 64) fp32 = the sums of z and z^2 per channel as ``ops_gemm.bn_statistics`` takes a
    producer's (None without ``want_stats``)."""
    L.require_cuda(prim, w)
    _check_map("ghost_tail", prim, 32)
    if tuple(w.shape) != (32, 1, 3, 3):
        raise L.P4CError(f"ghost_tail: a (32,1,3,3) depthwise weight expected, got {tuple(w.shape)}")
    return _GhostTail.apply(prim, w, bool(want_stats))


class _Merge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a0, a1, a2, a3, a4):
        maps = [a.contiguous() for a in (a0, a1, a2, a3, a4)]
        B, H, W, C = maps[0].shape
        out = torch.empty_like(maps[0])
        es = out.element_size()
        L.call("p4c_halfunet_merge_fwd", *[L.ptr(a) for a in maps], L.ptr(out), L.dtype_code(out.dtype), B, H, W, C, L.stream(out.device),
               alg_bytes=es * (sum(a.numel() for a in maps) + out.numel()))
        ctx.geom = (B, H, W, C)
        return out

    @staticmethod
    def backward(ctx, dS):
        B, H, W, C = ctx.geom
        dS = dS.contiguous()
        tx = [torch.empty(B, H, W >> k, C, dtype=torch.float32, device=dS.device) for k in (1, 2, 3, 4)]     # the x pass's fp32 sums
        da = [torch.empty(B, H >> k, W >> k, C, dtype=dS.dtype, device=dS.device) for k in (1, 2, 3, 4)]
        es = dS.element_size()
        L.call("p4c_halfunet_merge_bwd", L.ptr(dS), *[L.ptr(t) for t in tx], *[L.ptr(t) for t in da], L.dtype_code(dS.dtype), B, H, W, C,
               L.stream(dS.device), alg_bytes=es * (dS.numel() + sum(t.numel() for t in da)) + 2 * 4 * sum(t.numel() for t in tx))
        return (dS, *da)          # (the full-resolution level's gradient is dS itself: no copy)


def halfunet_merge(a0, a1, a2, a3, a4) -> torch.Tensor:
    """``a0 + sum_k F.interpolate(a_k, scale_factor=2**k, mode="bilinear", align_corners=False)`` for features-last maps a_k
    (B, H/2^k, W/2^k, 64), k = 0..4, H and W multiples of 16: summed in fp32, rounded once."""
    L.require_cuda(a0, a1, a2, a3, a4)
    _check_map("halfunet_merge", a0, a0.shape[-1])
    B, H, W, C = a0.shape
    for k, a in enumerate((a1, a2, a3, a4), 1):
        if a.dtype != a0.dtype or tuple(a.shape) != (B, H >> k, W >> k, C) or H % 16 or W % 16:
            raise L.P4CError(f"halfunet_merge: level {k} is {tuple(a.shape)} {a.dtype} under a {tuple(a0.shape)} {a0.dtype} map "
                             "(H and W multiples of 16, level k at 1/2^k of it)")
    return _Merge.apply(a0, a1, a2, a3, a4)


class _BNReluPool(torch.autograd.Function):
    """(act, pool) = relu(bn(z)) and its 2x2 max-pool, dense maps: unet's encoder tail with the skip written at ld = C"""

    @staticmethod
    def forward(ctx, z, stats, gamma, beta, bn, training):
        zc = z.contiguous()
        B, H, W, C = zc.shape
        dev = zc.device
        st = G.bn_statistics(zc, stats, bn, training)
        act = torch.empty_like(zc)
        pool = torch.empty(B, H // 2, W // 2, C, dtype=zc.dtype, device=dev)
        es = zc.element_size()
        L.call("p4c_unet_enc_tail_fwd", L.ptr(zc), L.ptr(st[2]), L.ptr(st[3]), L.ptr(act), C, L.ptr(pool), L.dtype_code(zc.dtype), B, H, W, C,
               L.stream(dev), alg_bytes=es * (zc.numel() * 2 + pool.numel()))
        ctx.save_for_backward(zc, st, act)
        ctx.training, ctx.has_affine = bool(training), gamma is not None
        ctx.set_materialize_grads(False)
        return act, pool

    @staticmethod
    def backward(ctx, dact, dpool):
        zc, st, act = ctx.saved_tensors
        B, H, W, C = zc.shape
        dev = zc.device
        dact = torch.zeros_like(zc) if dact is None else dact.contiguous()
        dpool = torch.zeros(B, H // 2, W // 2, C, dtype=zc.dtype, device=dev) if dpool is None else dpool.contiguous()
        nb = L.lib().p4c_unet_enc_tail_bwd_blocks(B, H, W, C)
        part = torch.empty(1, nb, 2, C, dtype=torch.float32, device=dev)
        dz = torch.empty_like(zc)
        es = zc.element_size()
        L.call("p4c_unet_enc_tail_bwd", L.ptr(zc), L.ptr(act), C, L.ptr(dact), C, L.ptr(dpool), L.ptr(st[0]), L.ptr(st[1]), L.ptr(dz), L.ptr(part),
               L.dtype_code(zc.dtype), B, H, W, C, L.stream(dev), alg_bytes=es * (zc.numel() * 4 + dpool.numel()))
        dy, dg, db = G.bn_tail_backward(zc, dz, part, nb, st, ctx.training, ctx.has_affine)
        return dy, None, dg, db, None, None


def bn_relu_pool(z: torch.Tensor, stats, bn):
    """(relu(bn(z)), max_pool2d(relu(bn(z)), 2)) for a features-last z (B,H,W,C), H and W even; ``bn``: what ops_gemm reads from an
    nn.BatchNorm2d; ``stats``: the producer's column sums or None."""
    L.require_cuda(z)
    B, H, W, C = z.shape
    if z.dtype not in (torch.float32, torch.bfloat16) or H % 2 or W % 2 or C % 4 or C > 1024:
        raise L.P4CError(f"bn_relu_pool: unsupported map {tuple(z.shape)} {z.dtype}")
    training = bn.training or bn.running_mean is None
    return _BNReluPool.apply(z, stats if training else None, bn.weight, bn.bias, bn, training)
