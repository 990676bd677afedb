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
point fails loudly.

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


def schedule(model):
    """[(kind, module name, module)] in the order DeepLabV3MI355X._forward_native calls its nodes (the bf16 route)"""
    s = [("patch", "encoder.conv1"), ("stem", "encoder.bn1")]
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


class Node:
    """one recorded call: kind, name, module (the live module), pre / post (deep copies of its batch norm before / right after the call),
    args (input clones), src (input name -> (node index, output index) of the recorded output it is), out (output clones), gout (the
    gradients the outputs received), gin (the Function's backward results), opts (the call's options), saved (tensors the node's ctx
    saved that a reference reads: the stem's routing table)"""

    def __init__(self, kind, name, module, args, opts):
        self.kind, self.name, self.module, self.args, self.opts = kind, name, module, args, opts
        bn = _norm_of(kind, module)
        self.pre = copy.deepcopy(bn) if bn is not None else None
        self.post = None
        self.src, self.out, self.gout, self.gin, self.saved = {}, None, None, None, {}

    @property
    def norm(self):
        return _norm_of(self.kind, self.module)

    def grad(self, slot):
        """the gradient this node's backward returned for input `slot`"""
        return self.gin[GRAD_SLOTS[self.kind][slot]]

    def params(self):
        """{slot: leaf parameter} of this node"""
        if self.kind in ("bn", "stem"):
            return {"gamma": self.module.weight, "beta": self.module.bias}
        if self.kind == "aspp":
            return {"w": self.module[1].weight, "gamma": self.module[2].weight, "beta": self.module[2].bias}
        if self.kind == "up":
            return {}
        ps = {"w": self.module.weight}
        if self.module.bias is not None:
            ps["b"] = self.module.bias
        return ps


class Recorder:
    """``with Recorder(model) as rec: y = model(x); y.backward(dy)`` -- rec.nodes in call order; the schedule is checked call by call
    and the node counts are asserted on exit"""

    def __init__(self, model):
        assert model.native, "the recorder follows the bf16 route (the fp32 flavour runs on library operations)"
        self.model = model
        self.expected = schedule(model)
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
        assert i < len(self.expected), f"node {i} ({kind}): more node calls than DeepLabV3MI355X makes ({len(self.expected)})"
        ekind, name, module = self.expected[i]
        assert kind == ekind, f"node {i}: expected {ekind} {name}, got a {kind} call"
        if kind in ("patch", "conv"):
            assert param_of(owner) is module.weight, f"{name}: the call's weight is not the model's {name}.weight"
        elif kind != "up":      # (the up-sampling has no module argument: its place in the schedule identifies it)
            assert owner is module, f"{name}: the call's module is not the model's {name}"
        node = Node(kind, name, module, {k: _clone(v) for k, v in args.items()}, opts)
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

    def _wrap_backward(self, fn_cls):
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

    def __enter__(self):
        from py4cast_amd import deeplabv3 as D
        from py4cast_amd import ops_gemm as G
        from py4cast_amd import ops_patch as P

        rec = self
        conv0, bn0, patch0 = G.conv2d_nhwc, G.batch_norm_act, D.DeepLabV3MI355X._patch
        stem0, aspp0, up0 = D.stem_tail, D.aspp_assemble, D.upsample_bilinear_ac

        def conv2d_nhwc(x, w, b=None, res=None, want_stats=False, passthrough=False, dilation=1):
            assert res is None, "DeepLabV3's convolutions take no residual operand (the residual goes to the batch norm)"
            node = rec._begin("conv", w, {"x": x, "w": w, "b": b},
                              {"want_stats": bool(want_stats), "passthrough": bool(passthrough), "dilation": int(dilation)})
            out = conv0(x, w, b, want_stats=want_stats, passthrough=passthrough, dilation=dilation)
            outs = list(out) if isinstance(out, tuple) else [out]
            y = outs[0]
            st = outs[1] if want_stats else None
            xp = outs[-1] if passthrough else None
            rec._end(node, [y, st, xp], y.grad_fn)
            return out

        def batch_norm_act(y, stats, bn, slope=1.0, res=None, res_passthrough=False, mul=None, mul_factor=1.0):
            assert not res_passthrough, "DeepLabV3's batch norms pass no residual on"
            node = rec._begin("bn", bn, {"y": y, "stats": stats, "res": res, "mul": mul}, {"slope": float(slope), "mul_factor": float(mul_factor)})
            out = bn0(y, stats, bn, slope=slope, res=res, mul=mul, mul_factor=mul_factor)
            rec._end(node, [out], out.grad_fn)
            return out

        def _patch(conv, x):
            k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
            assert conv.kernel_size[1] == k and conv.stride[1] == s and conv.padding[1] == p and conv.dilation == (1, 1)
            assert conv.bias is None
            node = rec._begin("patch", conv.weight, {"x": x, "w": conv.weight}, {"k": k, "stride": s, "pad": p})
            y, st = patch0(conv, x)
            rec._end(node, [y, st], y.grad_fn)
            return y, st

        def stem_tail(y, stats, bn):
            node = rec._begin("stem", bn, {"y": y, "stats": stats}, {})
            pool = stem0(y, stats, bn)
            node.saved["arg"] = pool.grad_fn.saved_tensors[2].clone() if pool.grad_fn is not None else None
            rec._end(node, [pool], pool.grad_fn)
            return pool

        def aspp_assemble(x, branches, pool_branch):
            node = rec._begin("aspp", pool_branch, {"x": x, **{f"a{k}": t for k, t in enumerate(branches)}, "w": pool_branch[1].weight}, {})
            buf = aspp0(x, branches, pool_branch)
            rec._end(node, [buf], buf.grad_fn)
            return buf

        def upsample_bilinear_ac(x, scale):
            node = rec._begin("up", None, {"x": x}, {"scale": int(scale)})
            out = up0(x, scale)
            rec._end(node, [out], out.grad_fn)
            return out

        self._mp = pytest.MonkeyPatch()
        self._mp.setattr(G, "conv2d_nhwc", conv2d_nhwc)
        self._mp.setattr(G, "batch_norm_act", batch_norm_act)
        self._mp.setattr(D.DeepLabV3MI355X, "_patch", staticmethod(_patch))
        self._mp.setattr(D, "stem_tail", stem_tail)
        self._mp.setattr(D, "aspp_assemble", aspp_assemble)
        self._mp.setattr(D, "upsample_bilinear_ac", upsample_bilinear_ac)
        for fn_cls in (G._Conv, G._BatchNormAct, P._PatchConv, D._StemTail, D._AsppAssemble, D._UpsampleAC):
            self._wrap_backward(fn_cls)
        return self

    def __exit__(self, exc_type, exc, tb):
        self._mp.undo()
        self._keep = []
        if exc_type is None:
            want = counts(self.model)
            got = {k: sum(n.kind == k for n in self.nodes) for k in KINDS}
            assert got == want, f"DeepLabV3 node calls {got}, expected {want}: a model change routes around the recorded entry points"
        return False
