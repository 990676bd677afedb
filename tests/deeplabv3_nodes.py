"""
Node-level oracle of the native DeepLabV3 (py4cast_amd/deeplabv3.py): a recorder of the network's node calls and float64 references of
each node -- the helpers of tests/test_deeplabv3_nodes_gpu.py (the device) and tests/test_deeplabv3_nodes_cpu.py (the references
themselves, composed into the whole network against tests/deeplabv3_reference.py).

Recorder: wraps the six entry points DeepLabV3MI355X._forward_native reaches (ops_gemm.conv2d_nhwc with its dilation / passthrough /
bias, ops_gemm.batch_norm_act with its residual and multiplier, DeepLabV3MI355X._patch -- the strided convolutions as ops_patch._PatchConv --,
deeplabv3.stem_tail, deeplabv3.aspp_assemble, deeplabv3.upsample_bilinear_ac) and the ``backward`` of their autograd Functions.  Per call,
in order: clones of the inputs, deep copies of the node's batch norm taken before and right after the call, the outputs, the gradient
each output receives in the backward (cloned on entry) together with the gradients the node returns, and which recorded output each
input is.  The calls themselves are untouched: same arguments, same kernels.  The expected call schedule is built from the model's
modules (``schedule``) and checked call by call; the counts are asserted on exit, so a model change that routes around a recorded entry
point fails loudly.  What differs between the three ResNet-encoder models -- the schedule, the module whose names are patched, the extra
node kinds -- comes from a ``Description``: DeepLabV3's here (the default), CustomUNet's in tests/customunet_nodes.py, DeepLabV3Plus's in
tests/deeplabv3plus_nodes.py; the references of their extra nodes (``dw_node``, ``upcat_node``, ``up2cat_node``, ``stemskip_node``) and the
``Composer`` their CPU tests build the whole network with stand beside DeepLabV3's below.

References: float64 on bf16-rounded operands (the GEMM weights rounded as the GEMM reads them; the ASPP pooling branch's 1x1 weight
and every batch-norm parameter as given: those kernels read fp32).  For a backward they take every decision from the values the device
STORED -- ReLU masks from the stored output > 0, the Dropout draw from the model's ``last_dropout_mask``, the stem's max-pool routing from
the ``arg`` table _StemTail saves (window index 0..8 per output and channel, first maximum wins) -- so that a gradient comparison never
crosses a decision; forward outputs are checked against the references' own decisions (a flip at |z| ~ rounding moves a value by about
the rounding, while a device mask would hide an output wrongly left at zero).  Features-last (B, H, W, C) throughout; every function
runs on CPU or GPU tensors alike.
"""
import copy
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from unet_nodes import _clone, _grads, _key, _leaf, param_of, running_update  # noqa: F401  (running_update: re-exported)

# ------------------------------------------------------------------------------------------------ float64 node references


def conv(x, w, b=None, stride=1, pad=0, dilation=1):
    """Conv2d(stride, padding, dilation) of a float64 features-last map x (B, H, W, Cx) with w (Co, Ci, k, k), Ci <= Cx (a wider map's
    extra channels meet zero weight columns, as DeepLabV3MI355X._patch pads the stem weight): one matmul per tap"""
    B, H, W, Cx = x.shape
    Co, Ci, k = w.shape[0], w.shape[1], w.shape[2]
    if Ci < Cx:
        w = F.pad(w, (0, 0, 0, 0, 0, Cx - Ci))
    Ho = (H + 2 * pad - dilation * (k - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dilation * (k - 1) - 1) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad)) if pad else x
    y = 0
    for ky in range(k):
        for kx in range(k):
            oy, ox = ky * dilation, kx * dilation
            xs = xp[:, oy: oy + stride * (Ho - 1) + 1: stride, ox: ox + stride * (Wo - 1) + 1: stride, :]
            y = y + (xs.reshape(-1, Cx) @ w[:, :, ky, kx].t()).view(B, Ho, Wo, Co)
    return y if b is None else y + b


def conv_node(x, w, b=None, stride=1, pad=0, dilation=1, dy=None, round_weight=True):
    """float64 convolution node: y, and with dy (y, dx, dw, db).  round_weight: the weight rounded to bf16 first, as the GEMM reads it
    (x is taken as given: the bf16 map, promoted).  dw has w's own shape (Ci columns; a wider map's padding channels get no gradient
    there)."""
    wd = w.detach().to(torch.bfloat16) if round_weight else w.detach()
    x64, w64, b64 = _leaf(x), _leaf(wd), _leaf(b)
    with torch.enable_grad():
        y = conv(x64, w64, b64, stride, pad, dilation)
    if dy is None:
        return y.detach()
    return (y.detach(),) + _grads(y, (x64, w64, b64), dy.double())


BNA = namedtuple("BNA", "out mask mean var var_unbiased dy dres dgamma dbeta")


def bn_act(y, gamma, beta, eps, slope=0.0, res=None, mul=None, factor=1.0, running=None, mask=None, dout=None):
    """float64 ``leaky_relu(BatchNorm2d(y) (+ res), slope) * mul[row group, channel] * factor`` of a features-last y: BNA.
    Training (running None): batch statistics over (B, H, W); eval: running = (mean, var).  mul (groups, C) with the groups equal
    consecutive runs of the B H W rows (DeepLabV3's Dropout: one group per pixel), None: no multiplier.  The LeakyReLU sign is z > 0
    unless `mask` is given (the device's stored output > 0: where mul is 0 the gradient is 0 whatever the sign).  With dout: the float64
    batch-norm backward of dout * mul * factor * sign', and dres = the residual's gradient (the same dz)."""
    C = y.shape[-1]
    r = y.detach().double().reshape(-1, C)
    N = r.shape[0]
    g, bt = gamma.detach().double(), beta.detach().double()
    if running is None:
        mean, var = r.mean(0), r.var(0, unbiased=False)
    else:
        mean, var = running[0].detach().double(), running[1].detach().double()
    rstd = torch.rsqrt(var + eps)
    xhat = (r - mean) * rstd
    z = xhat * g + bt
    if res is not None:
        z = z + res.detach().double().reshape(-1, C)
    if mul is None:
        m = torch.ones(1, C, dtype=torch.float64, device=y.device)
    else:
        m = mul.detach().double().repeat_interleave(N // mul.shape[0], 0) * factor
    pos = (z > 0) if mask is None else mask.reshape(-1, C)
    sign = torch.where(pos, z.new_tensor(1.0), z.new_tensor(float(slope)))
    out = (z * sign * m).view(y.shape)
    dy = dres = dgamma = dbeta = None
    if dout is not None:
        dz = dout.detach().double().reshape(-1, C) * m * sign
        dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
        dyr = g * rstd * (dz - dbeta / N - xhat * (dgamma / N)) if running is None else g * rstd * dz
        dy = dyr.view(y.shape)
        dres = dz.view(y.shape) if res is not None else None
    vu = r.var(0, unbiased=True) if running is None and N > 1 else None
    return BNA(out, pos.view(y.shape), mean, var, vu, dy, dres, dgamma, dbeta)


def pool_arg(a):
    """the window index (ky 3 + kx, uint8) of each 3x3 / 2 / padding-1 window's first maximum of a (B, H, W, C) in row-major order
    (torch's max_pool2d rule, the device's ``arg`` table)"""
    B, H, W, C = a.shape
    _, idx = F.max_pool2d(a.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    idx = idx.permute(0, 2, 3, 1)
    Ho, Wo = idx.shape[1], idx.shape[2]
    oy = torch.arange(Ho, device=a.device).view(1, Ho, 1, 1)
    ox = torch.arange(Wo, device=a.device).view(1, 1, Wo, 1)
    return ((idx // W - (2 * oy - 1)) * 3 + (idx % W - (2 * ox - 1))).to(torch.uint8)


STEM = namedtuple("STEM", "pool pool_at_arg mean var var_unbiased dy dgamma dbeta")


def _pool_windows(a, arg):
    """the value of a (B, H, W, C) at each 3x3 / 2 / padding-1 window's position `arg` (B, Ho, Wo, C) (window index ky 3 + kx)"""
    B, H, W, C = a.shape
    Ho, Wo = arg.shape[1], arg.shape[2]
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    out = torch.zeros(B, Ho, Wo, C, dtype=a.dtype, device=a.device)
    for k in range(9):
        ky, kx = divmod(k, 3)
        sel = arg.long() == k
        out = torch.where(sel, ap[:, ky: ky + 2 * (Ho - 1) + 1: 2, kx: kx + 2 * (Wo - 1) + 1: 2, :], out)
    return out


def stem_node(y, gamma, beta, eps, running=None, arg=None, pool_stored=None, dpool=None):
    """float64 stem tail: pool = max_pool2d(relu(bn(y)), 3, 2, 1) on this reference's own values (torch's rule: first maximum in
    row-major order), and with `arg` (the device's routing table) the reference's activations at the device's chosen positions.  With
    dpool: the backward with the routing from `arg` and the ReLU mask from the stored pool > 0 (the routed pixel's activation IS the
    window's pooled value)."""
    b = bn_act(y, gamma, beta, eps, slope=0.0, running=running)
    a = b.out
    pool = F.max_pool2d(a.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    at_arg = None if arg is None else _pool_windows(a, arg)
    dy = dgamma = dbeta = None
    if dpool is not None:
        B, H, W, C = y.shape
        Ho, Wo = arg.shape[1], arg.shape[2]
        g = dpool.double() * (pool_stored.double() > 0)
        dap = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64, device=y.device)
        for k in range(9):
            ky, kx = divmod(k, 3)
            dap[:, ky: ky + 2 * (Ho - 1) + 1: 2, kx: kx + 2 * (Wo - 1) + 1: 2, :] += torch.where(arg.long() == k, g, torch.zeros_like(g))
        da = dap[:, 1: H + 1, 1: W + 1, :]
        bb = bn_act(y, gamma, beta, eps, slope=1.0, running=running, dout=da)
        dy, dgamma, dbeta = bb.dy, bb.dgamma, bb.dbeta
    return STEM(pool, at_arg, b.mean, b.var, b.var_unbiased, dy, dgamma, dbeta)


ASPP = namedtuple("ASPP", "buf pooled mean var var_unbiased dx dbranches dw dgamma dbeta")


def aspp_node(x, branches, w, gamma, beta, eps, running=None, pooled_stored=None, dbuf=None):
    """float64 ASPP assembly: buf = [a0 | a1 | a2 | a3 | relu(bn_B(mean_hw(x) W^T))] with the pooling branch broadcast over the map
    (its batch norm over the B samples; w (D, C, 1, 1) as given -- the kernel reads the fp32 master); pooled (B, D).  With dbuf: the
    backward, the ReLU mask from the stored pooled values > 0 (pooled_stored (B, D))."""
    B, H, W, C = x.shape
    D = w.shape[0]
    mean = x.detach().double().mean((1, 2))
    w2 = w.detach().double().reshape(D, C)
    z = mean @ w2.t()
    b = bn_act(z.view(B, 1, 1, D), gamma, beta, eps, slope=0.0, running=running)
    pooled = b.out.view(B, D)
    buf = torch.cat([t.detach().double() for t in branches] + [pooled.view(B, 1, 1, D).expand(B, H, W, D)], -1)
    dx = dbr = dw = dgamma = dbeta = None
    if dbuf is not None:
        d = dbuf.detach().double()
        dbr = [d[..., k * D: (k + 1) * D] for k in range(4)]
        dp = d[..., 4 * D:].sum((1, 2))
        bb = bn_act(z.view(B, 1, 1, D), gamma, beta, eps, slope=0.0, running=running, mask=pooled_stored.view(B, 1, 1, D) > 0,
                    dout=dp.view(B, 1, 1, D))
        dz = bb.dy.view(B, D)
        dw = (dz.t() @ mean).view(w.shape)
        dx = (dz @ w2 / (H * W)).view(B, 1, 1, C).expand(B, H, W, C)
        dgamma, dbeta = bb.dgamma, bb.dbeta
    return ASPP(buf, pooled, b.mean, b.var, b.var_unbiased, dx, dbr, dw, dgamma, dbeta)


def upsample_node(x, scale=8, dout=None):
    """float64 F.interpolate(scale_factor=scale, mode="bilinear", align_corners=True) of a features-last map; with dout (out, dx)"""
    x64 = _leaf(x)
    with torch.enable_grad():
        out = F.interpolate(x64.permute(0, 3, 1, 2), scale_factor=scale, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    if dout is None:
        return out.detach()
    return out.detach(), _grads(out, (x64,), dout.double())[0]


# ---- the nodes DeepLabV3Plus (tests/deeplabv3plus_nodes.py) and CustomUNet (tests/customunet_nodes.py) add

DW = namedtuple("DW", "ys dx dws")


def dw_node(x, ws, rates, dys=None):
    """float64 depthwise 3x3 at R rates: ys[r] = F.conv2d(x, w_r, padding = dilation = d_r, groups = C) of a features-last x with the
    (C, 1, 3, 3) weights AS GIVEN (the kernel reads the fp32 masters and rounds no weight).  With dys: the adjoint written out tap by
    tap on zero-padded maps -- dx = the sum over the rates of sum_t w_r[t] dy_r[p - off_t], dws[r][c, t] = sum_p dy_r[p] x[p + off_t]
    (tests/test_deeplabv3plus_nodes_cpu.py holds it to the autograd of F.conv2d, rates beyond the map included)."""
    B, H, W, C = x.shape
    x64 = x.detach().double()
    w64 = [w.detach().double() for w in ws]
    xn = x64.permute(0, 3, 1, 2)
    ys = [F.conv2d(xn, w, padding=d, dilation=d, groups=C).permute(0, 2, 3, 1) for w, d in zip(w64, rates)]
    if dys is None:
        return DW(ys, None, None)
    dx, dws = 0, []
    for w, d, dy in zip(w64, rates, dys):
        g = dy.detach().double()
        gp, xp = F.pad(g, (0, 0, d, d, d, d)), F.pad(x64, (0, 0, d, d, d, d))
        dw = torch.empty(C, 9, dtype=torch.float64, device=x.device)
        for ky in range(3):
            for kx in range(3):
                # y[p] takes x[p + (ky - 1, kx - 1) d]: dx[p] takes dy[p - that offset], dw the product summed over the map
                dx = dx + w[:, 0, ky, kx] * gp[:, (2 - ky) * d: (2 - ky) * d + H, (2 - kx) * d: (2 - kx) * d + W, :]
                dw[:, ky * 3 + kx] = (g * xp[:, ky * d: ky * d + H, kx * d: kx * d + W, :]).sum((0, 1, 2))
        dws.append(dw.view(C, 1, 3, 3))
    return DW(ys, dx, dws)


def upcat_node(a, skip, scale, ld, dout=None):
    """float64 ``[F.interpolate(a, scale, bilinear, align_corners=True) | skip | zeros up to ld]``; with dout (out, da, dskip): da the
    up-sampling's adjoint of dout's first Ca channels, dskip the slice"""
    Ca, Cs = a.shape[-1], skip.shape[-1]
    up = upsample_node(a, scale)
    out = torch.cat([up, skip.detach().double(), up.new_zeros(*up.shape[:3], ld - Ca - Cs)], -1)
    if dout is None:
        return out
    d = dout.detach().double()
    return out, upsample_node(a, scale, dout=d[..., :Ca])[1], d[..., Ca: Ca + Cs]


def up2cat_node(x, skip, dout=None):
    """float64 ``[nearest_x2(x) | skip]`` (skip None: the up-sampling alone; for up2_into: skip = the buffer's channels from Cx on);
    with dout (out, dx, dskip): dx the sum of the four, dskip the slice (None without a skip)"""
    Cx = x.shape[-1]
    up = x.detach().double().repeat_interleave(2, 1).repeat_interleave(2, 2)
    out = up if skip is None else torch.cat([up, skip.detach().double()], -1)
    if dout is None:
        return out
    d = dout.detach().double()
    B, H2, W2, _ = d.shape
    dx = d[..., :Cx].reshape(B, H2 // 2, 2, W2 // 2, 2, Cx).sum((2, 4))
    return out, dx, (None if skip is None else d[..., Cx:])


STEMSKIP = namedtuple("STEMSKIP", "act pool pool_at_arg mean var var_unbiased dy dgamma dbeta")


def stemskip_node(y, gamma, beta, eps, running=None, arg=None, act_stored=None, dpool=None, dskip=None):
    """stem_node with the activated map as a second output: act = relu(bn(y)), pool = max_pool2d(act, 3, 2, 1).  With dpool and dskip:
    the backward with the routing from `arg` (the device's table) and dskip added BEFORE the ReLU mask, taken from the stored
    activation > 0 (act_stored): dz = (dskip + the dpool of the windows that chose the pixel) [act > 0]."""
    b = bn_act(y, gamma, beta, eps, slope=0.0, running=running)
    a = b.out
    pool = F.max_pool2d(a.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    at_arg = None if arg is None else _pool_windows(a, arg)
    dy = dgamma = dbeta = None
    if dpool is not None:
        B, H, W, C = y.shape
        Ho, Wo = arg.shape[1], arg.shape[2]
        g = dpool.detach().double()
        dap = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64, device=y.device)
        for k in range(9):
            ky, kx = divmod(k, 3)
            dap[:, ky: ky + 2 * (Ho - 1) + 1: 2, kx: kx + 2 * (Wo - 1) + 1: 2, :] += torch.where(arg.long() == k, g, torch.zeros_like(g))
        da = (dap[:, 1: H + 1, 1: W + 1, :] + dskip.detach().double()) * (act_stored.detach().double() > 0)
        bb = bn_act(y, gamma, beta, eps, slope=1.0, running=running, dout=da)
        dy, dgamma, dbeta = bb.dy, bb.dgamma, bb.dbeta
    return STEMSKIP(a, pool, at_arg, b.mean, b.var, b.var_unbiased, dy, dgamma, dbeta)


# ------------------------------------------------------------------------------------------------ the recorder

# node kinds: "patch" (DeepLabV3MI355X._patch: ops_patch._PatchConv), "conv" (conv2d_nhwc), "bn" (batch_norm_act), "stem" (stem_tail),
# "aspp" (aspp_assemble), "up" (upsample_bilinear_ac)
KINDS = ("patch", "conv", "bn", "stem", "aspp", "up")

# per kind: the Function's backward results that are gradients of the named inputs
GRAD_SLOTS = {"patch": {"x": 0, "w": 1}, "conv": {"x": 0, "w": 1, "b": 2}, "bn": {"y": 0, "gamma": 2, "beta": 3, "res": 4},
              "stem": {"y": 0, "gamma": 2, "beta": 3}, "up": {"x": 0},
              "aspp": {"x": 0, "a0": 1, "a1": 2, "a2": 3, "a3": 4, "w": 5, "gamma": 6, "beta": 7}}

# the inputs whose gradients flow on to a producer
DIFF_INPUTS = {"patch": ("x",), "conv": ("x",), "bn": ("y", "res"), "stem": ("y",), "aspp": ("x", "a0", "a1", "a2", "a3"), "up": ("x",)}


def encoder_schedule(model):
    """[(kind, module name)] of the stem's convolution and the four ResNet layers, in the order ``_block`` calls its nodes (the stem
    tail, whose kind differs between the models, goes between entry 0 and the rest)"""
    s = [("patch", "encoder.conv1")]
    enc = model.encoder
    for li in range(1, 5):
        for j, blk in enumerate(getattr(enc, f"layer{li}")):
            p = f"encoder.layer{li}.{j}"
            if blk.downsample is not None:
                kind = "patch" if blk.conv1.stride[0] != 1 else "conv"
                s += [(kind, f"{p}.conv1"), (kind, f"{p}.downsample.0"), ("bn", f"{p}.downsample.1")]
            else:
                s.append(("conv", f"{p}.conv1"))
            s += [("bn", f"{p}.bn1"), ("conv", f"{p}.conv2"), ("bn", f"{p}.bn2")]
    return s


def schedule(model):
    """[(kind, module name, module)] in the order DeepLabV3MI355X._forward_native calls its nodes (the bf16 route)"""
    s = encoder_schedule(model)
    s.insert(1, ("stem", "encoder.bn1"))
    for i in range(4):
        s += [("conv", f"decoder.0.convs.{i}.0"), ("bn", f"decoder.0.convs.{i}.1")]
    s += [("aspp", "decoder.0.convs.4"), ("conv", "decoder.0.project.0"), ("bn", "decoder.0.project.1"), ("conv", "decoder.1"),
          ("bn", "decoder.2"), ("conv", "segmentation_head.0"), ("up", "segmentation_head.1")]
    return [(k, n, model.get_submodule(n)) for k, n in s]


def counts(model):
    return {k: sum(e[0] == k for e in schedule(model)) for k in KINDS}


def _norm_of(kind, module):
    """the batch norm a node owns (None for convolutions / up-sampling)"""
    if kind in ("bn", "stem"):
        return module
    return module[2] if kind == "aspp" else None


class Description:
    """What the Recorder needs to know about one of the three ResNet-encoder models.  This one is DeepLabV3's; tests/customunet_nodes.py
    and tests/deeplabv3plus_nodes.py derive theirs: the schedule, the names their module binds (``install``) and their extra node kinds
    (``kinds`` / ``grad_slots`` / ``diff_inputs`` / ``norm_of`` / ``params`` / ``check_owner``)."""

    label = "DeepLabV3MI355X"
    kinds, grad_slots, diff_inputs = KINDS, GRAD_SLOTS, DIFF_INPUTS

    def schedule(self, model):
        return schedule(model)

    def counts(self, model):
        return {k: sum(e[0] == k for e in self.schedule(model)) for k in self.kinds}

    def norm_of(self, kind, module):
        return _norm_of(kind, module)

    def params(self, node):
        if node.kind in ("bn", "stem"):
            return {"gamma": node.module.weight, "beta": node.module.bias}
        if node.kind == "aspp":
            return {"w": node.module[1].weight, "gamma": node.module[2].weight, "beta": node.module[2].bias}
        if node.kind == "up":
            return {}
        ps = {"w": node.module.weight}
        if node.module.bias is not None:
            ps["b"] = node.module.bias
        return ps

    def check_owner(self, kind, name, owner, module):
        """the call's weight / module argument is the scheduled module's"""
        if kind in ("patch", "conv"):
            assert param_of(owner) is module.weight, f"{name}: the call's weight is not the model's {name}.weight"
        elif kind != "up":      # (the up-sampling has no module argument: its place in the schedule identifies it)
            assert owner is module, f"{name}: the call's module is not the model's {name}"

    def install(self, rec):
        """patch the names this model's module reaches its nodes through (ops_gemm's two are the Recorder's own) and wrap the
        ``backward`` of their Functions"""
        from py4cast_amd import deeplabv3 as D

        rec.patch(D.DeepLabV3MI355X, "_patch", staticmethod(rec.wrap_patch(D.DeepLabV3MI355X._patch)))
        rec.patch(D, "stem_tail", rec.wrap_stem(D.stem_tail))
        rec.patch(D, "aspp_assemble", rec.wrap_aspp(D.aspp_assemble))
        rec.patch(D, "upsample_bilinear_ac", rec.wrap_up(D.upsample_bilinear_ac))
        for fn_cls in (D._StemTail, D._AsppAssemble, D._UpsampleAC):
            rec.wrap_backward(fn_cls)


class Node:
    """one recorded call: kind, name, module (the live module), pre / post (deep copies of its batch norm before / right after the call),
    args (input clones), src (input name -> (node index, output index) of the recorded output it is), out (output clones), gout (the
    gradients the outputs received), gin (the Function's backward results), opts (the call's options), saved (tensors the node's ctx
    saved that a reference reads: the stem's routing table)"""

    def __init__(self, kind, name, module, args, opts, desc=None):
        self.kind, self.name, self.module, self.args, self.opts = kind, name, module, args, opts
        self.desc = desc or Description()
        bn = self.desc.norm_of(kind, module)
        self.pre = copy.deepcopy(bn) if bn is not None else None
        self.post = None
        self.src, self.out, self.gout, self.gin, self.saved = {}, None, None, None, {}

    @property
    def norm(self):
        return self.desc.norm_of(self.kind, self.module)

    def grad(self, slot):
        """the gradient this node's backward returned for input `slot`"""
        return self.gin[self.desc.grad_slots[self.kind][slot]]

    def params(self):
        """{slot: leaf parameter} of this node"""
        return self.desc.params(self)


class Recorder:
    """``with Recorder(model) as rec: y = model(x); y.backward(dy)`` -- rec.nodes in call order; the schedule is checked call by call
    and the node counts are asserted on exit.  ``desc``: the model's Description (default: DeepLabV3's)."""

    def __init__(self, model, desc=None):
        assert model.native, "the recorder follows the bf16 route (the fp32 flavour runs on library operations)"
        self.model = model
        self.desc = desc or Description()
        self.expected = self.desc.schedule(model)
        self.nodes = []
        self._ctx = {}
        self._keep = []
        self._made = {}

    def __getitem__(self, name):
        for n in self.nodes:
            if n.name == name:
                return n
        raise KeyError(name)

    # -------------------------------------------------------------- forward side
    def _begin(self, kind, owner, args, opts):
        i = len(self.nodes)
        assert i < len(self.expected), f"node {i} ({kind}): more node calls than {self.desc.label} makes ({len(self.expected)})"
        ekind, name, module = self.expected[i]
        assert kind == ekind, f"node {i}: expected {ekind} {name}, got a {kind} call"
        self.desc.check_owner(kind, name, owner, module)
        node = Node(kind, name, module, {k: _clone(v) for k, v in args.items()}, opts, self.desc)
        for k, v in args.items():
            if isinstance(v, torch.Tensor) and _key(v) in self._made:
                node.src[k] = self._made[_key(v)]
        return node

    def _end(self, node, outs, ctx):
        node.out = [_clone(o) for o in outs]
        if node.pre is not None:
            node.post = copy.deepcopy(node.norm)
        i = len(self.nodes)
        self.nodes.append(node)
        for j, o in enumerate(outs):
            if isinstance(o, torch.Tensor):
                self._made[_key(o)] = (i, j)
        if ctx is not None:
            self._ctx[id(ctx)] = node
            self._keep.append(ctx)

    def patch(self, owner, name, value):
        self._mp.setattr(owner, name, value)

    def wrap_backward(self, fn_cls):
        orig = fn_cls.__dict__["backward"].__func__
        rec = self

        def backward(ctx, *grads):
            node = rec._ctx.get(id(ctx))
            if node is not None:
                node.gout = [_clone(g) for g in grads]
            res = orig(ctx, *grads)
            if node is not None:
                node.gin = [_clone(r) if isinstance(r, torch.Tensor) else None for r in res]
            return res

        self._mp.setattr(fn_cls, "backward", staticmethod(backward))

    # -------------------------------------------------------------- the wrappers of the entry points the three models share
    def wrap_conv(self, conv0):
        rec = self

        def conv2d_nhwc(x, w, b=None, res=None, want_stats=False, passthrough=False, dilation=1):
            assert res is None, f"{rec.desc.label}'s convolutions take no residual operand (the residual goes to the batch norm)"
            node = rec._begin("conv", w, {"x": x, "w": w, "b": b},
                              {"want_stats": bool(want_stats), "passthrough": bool(passthrough), "dilation": int(dilation)})
            out = conv0(x, w, b, want_stats=want_stats, passthrough=passthrough, dilation=dilation)
            outs = list(out) if isinstance(out, tuple) else [out]
            y = outs[0]
            st = outs[1] if want_stats else None
            xp = outs[-1] if passthrough else None
            rec._end(node, [y, st, xp], y.grad_fn)
            return out

        return conv2d_nhwc

    def wrap_bn(self, bn0):
        rec = self

        def batch_norm_act(y, stats, bn, slope=1.0, res=None, res_passthrough=False, mul=None, mul_factor=1.0):
            assert not res_passthrough, f"{rec.desc.label}'s batch norms pass no residual on"
            node = rec._begin("bn", bn, {"y": y, "stats": stats, "res": res, "mul": mul}, {"slope": float(slope), "mul_factor": float(mul_factor)})
            out = bn0(y, stats, bn, slope=slope, res=res, mul=mul, mul_factor=mul_factor)
            rec._end(node, [out], out.grad_fn)
            return out

        return batch_norm_act

    def wrap_patch(self, patch0):
        rec = self

        def _patch(conv, x):
            k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
            assert conv.kernel_size[1] == k and conv.stride[1] == s and conv.padding[1] == p and conv.dilation == (1, 1)
            assert conv.bias is None
            node = rec._begin("patch", conv.weight, {"x": x, "w": conv.weight}, {"k": k, "stride": s, "pad": p})
            y, st = patch0(conv, x)
            rec._end(node, [y, st], y.grad_fn)
            return y, st

        return _patch

    def wrap_stem(self, stem0):
        rec = self

        def stem_tail(y, stats, bn):
            node = rec._begin("stem", bn, {"y": y, "stats": stats}, {})
            pool = stem0(y, stats, bn)
            node.saved["arg"] = pool.grad_fn.saved_tensors[2].clone() if pool.grad_fn is not None else None
            rec._end(node, [pool], pool.grad_fn)
            return pool

        return stem_tail

    def wrap_aspp(self, aspp0):
        rec = self

        def aspp_assemble(x, branches, pool_branch):
            node = rec._begin("aspp", pool_branch, {"x": x, **{f"a{k}": t for k, t in enumerate(branches)}, "w": pool_branch[1].weight}, {})
            buf = aspp0(x, branches, pool_branch)
            rec._end(node, [buf], buf.grad_fn)
            return buf

        return aspp_assemble

    def wrap_up(self, up0):
        rec = self

        def upsample_bilinear_ac(x, scale):
            node = rec._begin("up", None, {"x": x}, {"scale": int(scale)})
            out = up0(x, scale)
            rec._end(node, [out], out.grad_fn)
            return out

        return upsample_bilinear_ac

    def __enter__(self):
        from py4cast_amd import ops_gemm as G
        from py4cast_amd import ops_patch as P

        self._mp = pytest.MonkeyPatch()
        # (every model reaches these two as G.<name>: one patch covers the three)
        self._mp.setattr(G, "conv2d_nhwc", self.wrap_conv(G.conv2d_nhwc))
        self._mp.setattr(G, "batch_norm_act", self.wrap_bn(G.batch_norm_act))
        for fn_cls in (G._Conv, G._BatchNormAct, P._PatchConv):
            self.wrap_backward(fn_cls)
        self.desc.install(self)
        return self

    def __exit__(self, exc_type, exc, tb):
        self._mp.undo()
        self._keep = []
        if exc_type is None:
            want = self.desc.counts(self.model)
            got = {k: sum(n.kind == k for n in self.nodes) for k in self.desc.kinds}
            assert got == want, f"{self.desc.label} node calls {got}, expected {want}: a model change routes around the recorded entry points"
        return False


# ------------------------------------------------------------------------------------------------ composing the references (CPU tests)
class Composer:
    """the bookkeeping of a hand composition of the node references into a float64 restatement `ref` (its train / eval mode): parameter
    gradients by name (``put``; several contributions add), each batch norm's node result by module name (``bna``), and the four ResNet
    layers forward and backward -- what tests/test_customunet_nodes_cpu.py and tests/test_deeplabv3plus_nodes_cpu.py share"""

    def __init__(self, ref):
        self.names = {id(p): n for n, p in ref.named_parameters()}
        self.mods = {id(m): n for n, m in ref.named_modules()}
        self.grads, self.norms, self.train = {}, {}, ref.training

    def put(self, p, g):
        n = self.names[id(p)]
        self.grads[n] = g if n not in self.grads else self.grads[n] + g

    def running(self, bn):
        return None if self.train else (bn.running_mean, bn.running_var)

    def bna(self, y, bn, slope=0.0, **kw):
        r = bn_act(y, bn.weight, bn.bias, bn.eps, slope=slope, running=self.running(bn), **kw)
        self.norms[self.mods[id(bn)]] = r
        return r

    def blocks_forward(self, enc, geom, h):
        """the BasicBlocks of layer1 .. layer4 (geom: (stride, dilation) per layer) on h: (per-block records, each layer's output)"""
        blocks, feats = [], []
        for li, (s, d) in enumerate(geom):
            layer = getattr(enc, f"layer{li + 1}")
            for j, blk in enumerate(layer):
                st = s if j == 0 else 1
                rec = {"x": h, "blk": blk, "st": st, "d": d, "layer": li, "last": j == len(layer) - 1}
                rec["c1"] = conv_node(h, blk.conv1.weight, stride=st, pad=d, dilation=d, round_weight=False)
                if hasattr(blk, "downsample"):
                    rec["cd"] = conv_node(h, blk.downsample[0].weight, stride=st, round_weight=False)
                    rec["bd"] = self.bna(rec["cd"], blk.downsample[1], slope=1.0)
                    idn = rec["bd"].out
                else:
                    idn = h
                rec["idn"] = idn
                rec["b1"] = self.bna(rec["c1"], blk.bn1)
                rec["c2"] = conv_node(rec["b1"].out, blk.conv2.weight, pad=d, dilation=d, round_weight=False)
                rec["b2"] = self.bna(rec["c2"], blk.bn2, res=idn)
                h = rec["b2"].out
                blocks.append(rec)
            feats.append(h)
        return blocks, feats

    def blocks_backward(self, blocks, dh, extra):
        """the blocks in reverse from dh, the gradient of layer4's output; extra {layer index: the gradient that layer's output receives
        from its consumers outside the encoder (the decoder's skips), added to the next layer's as autograd adds them}: the gradient
        of the stem's pooled map"""
        put = self.put
        for rec in reversed(blocks):
            blk, st, d = rec["blk"], rec["st"], rec["d"]
            if rec["last"] and rec["layer"] in extra:
                dh = dh + extra[rec["layer"]]
            b2 = self.bna(rec["c2"], blk.bn2, res=rec["idn"], mask=rec["b2"].mask, dout=dh)
            put(blk.bn2.weight, b2.dgamma)
            put(blk.bn2.bias, b2.dbeta)
            _, db1, dw, _ = conv_node(rec["b1"].out, blk.conv2.weight, pad=d, dilation=d, dy=b2.dy, round_weight=False)
            put(blk.conv2.weight, dw)
            b1 = self.bna(rec["c1"], blk.bn1, mask=rec["b1"].mask, dout=db1)
            put(blk.bn1.weight, b1.dgamma)
            put(blk.bn1.bias, b1.dbeta)
            _, dx1, dw, _ = conv_node(rec["x"], blk.conv1.weight, stride=st, pad=d, dilation=d, dy=b1.dy, round_weight=False)
            put(blk.conv1.weight, dw)
            if "cd" in rec:
                bd = self.bna(rec["cd"], blk.downsample[1], slope=1.0, dout=b2.dres)
                put(blk.downsample[1].weight, bd.dgamma)
                put(blk.downsample[1].bias, bd.dbeta)
                _, dxd, dw, _ = conv_node(rec["x"], blk.downsample[0].weight, stride=st, dy=bd.dy, round_weight=False)
                put(blk.downsample[0].weight, dw)
                dh = dx1 + dxd                 # the block input's two consumers
            else:
                dh = dx1 + b2.dres             # the identity edge (conv1's passthrough on the device)
        return dh
