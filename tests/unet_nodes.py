"""
Node-level oracle of the native UNet (py4cast_amd/unet.py): a recorder of the network's node calls and float64 references of each node
-- the helpers of tests/test_unet_nodes_gpu.py (the device) and tests/test_unet_nodes_cpu.py (the references themselves).

Recorder: wraps the four entry points UNetMI355X calls (ops_gemm.conv2d_nhwc, ops_gemm.batch_norm_act, unet.enc_tail,
unet.upconv_into) and the ``backward`` of their autograd Functions.  Per call, in order: clones of the inputs, a deep copy of the layer's
batch norm taken before the call, the outputs, and the gradient each output receives in the backward (cloned on entry: the transposed
convolution's backward zeroes its incoming gradient in place) together with the gradients the node returns; and which recorded output
each input is.  The calls themselves are untouched: same arguments, same kernels.

References: float64 on bf16-rounded operands (as tests/test_gemm_gpu.py's conv_ref).  For a backward they can take every decision
(ReLU mask, max-pool routing) from the values the device STORED, so that a gradient comparison never crosses a decision -- the
network-level bars of tests/test_unet_gpu.py had to open up because it does; forward outputs are checked against the references' own
decisions (a flip at |z| ~ rounding moves a value by about the rounding, while a device mask would hide an output wrongly left at zero).  Features-last (B, H, W, C) throughout; every function runs on CPU or GPU tensors alike.
"""
import copy
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------------------ float64 node references


def _grads(out, inputs, dout):
    """gradients of `out` with respect to `inputs` (None entries stay None) for the incoming gradient `dout`"""
    live = [t for t in inputs if t is not None]
    got = iter(torch.autograd.grad(out, live, dout))
    return tuple(None if t is None else next(got) for t in inputs)


def _leaf(t):
    return None if t is None else t.detach().double().requires_grad_(True)


def conv(x, w, b=None):
    """'same' 3x3 / 1x1 convolution of a float64 features-last map x (B, H, W, Ci) with w (Co, Ci, k, k): one matmul per tap"""
    B, H, W, Ci = x.shape
    Co, k = w.shape[0], w.shape[2]
    if k == 1:
        y = (x.reshape(-1, Ci) @ w.reshape(Co, Ci).t()).view(B, H, W, Co)
    else:
        xp = F.pad(x, (0, 0, 1, 1, 1, 1))
        y = 0
        for ky in range(3):
            for kx in range(3):
                y = y + (xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Ci) @ w[:, :, ky, kx].t()).view(B, H, W, Co)
    return y if b is None else y + b


def conv_node(x, w, b=None, dy=None, round_weight=True):
    """float64 convolution node: y, and with dy (y, dx, dw, db).  round_weight: the weight rounded to bf16 first, as the GEMM reads it
    (x is taken as given: the bf16 map, promoted)"""
    wd = w.detach().to(torch.bfloat16) if round_weight else w.detach()
    x64, w64, b64 = _leaf(x), _leaf(wd), _leaf(b)
    with torch.enable_grad():
        y = conv(x64, w64, b64)
    if dy is None:
        return y.detach()
    return (y.detach(),) + _grads(y, (x64, w64, b64), dy.double())


def upconv(x, w, b=None):
    """ConvTranspose2d(kernel 2, stride 2) of a float64 features-last x (B, H, W, Ci) with w (Ci, Co, 2, 2): (B, 2H, 2W, Co)"""
    B, H, W, Ci = x.shape
    Co = w.shape[1]
    y = (x.reshape(-1, Ci) @ w.reshape(Ci, Co * 4)).view(B, H, W, Co, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * H, 2 * W, Co)
    return y if b is None else y + b


def upconv_node(x, w, b=None, dup=None, round_weight=True):
    """float64 transposed-convolution node: up, and with dup (the gradient of up) (up, dx, dw, db)"""
    wd = w.detach().to(torch.bfloat16) if round_weight else w.detach()
    x64, w64, b64 = _leaf(x), _leaf(wd), _leaf(b)
    with torch.enable_grad():
        y = upconv(x64, w64, b64)
    if dup is None:
        return y.detach()
    return (y.detach(),) + _grads(y, (x64, w64, b64), dup.double())


BN = namedtuple("BN", "out mask mean var var_unbiased dy dgamma dbeta")


def bn_node(y, gamma, beta, eps, mask=None, dout=None, running=None):
    """float64 BatchNorm2d + ReLU of a features-last y.  Training (running None): batch statistics; eval: running = (mean, var).
    out = z where mask, else 0; mask = z > 0 unless given (the device's stored output > 0: the kernels decide on it, csrc/inorm.hip
    MODE 1).  With dout: the float64 batch-norm backward of dout * mask."""
    C = y.shape[-1]
    r = y.detach().double().reshape(-1, C)
    N = r.shape[0]
    g = gamma.detach().double()
    bt = beta.detach().double()
    if running is None:
        mean, var = r.mean(0), r.var(0, unbiased=False)
    else:
        mean, var = running[0].detach().double(), running[1].detach().double()
    rstd = torch.rsqrt(var + eps)
    xhat = (r - mean) * rstd
    z = xhat * g + bt
    m = (z > 0) if mask is None else mask.reshape(-1, C)
    out = torch.where(m, z, torch.zeros_like(z)).view(y.shape)
    dy = dgamma = dbeta = None
    if dout is not None:
        dz = torch.where(m, dout.detach().double().reshape(-1, C), torch.zeros_like(z))
        dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
        dyr = g * rstd * (dz - dbeta / N - xhat * (dgamma / N)) if running is None else g * rstd * dz
        dy = dyr.view(y.shape)
    vu = r.var(0, unbiased=True) if running is None and N > 1 else None
    return BN(out, m.view(y.shape), mean, var, vu, dy, dgamma, dbeta)


def _windows(t):
    """(B, H, W, C) -> (B, H/2, W/2, C, 4): the 2x2 windows in scan order (0,0) (0,1) (1,0) (1,1)"""
    B, H, W, C = t.shape
    return t.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)


def _unwindows(t):
    B, Ho, Wo, C, _ = t.shape
    return t.reshape(B, Ho, Wo, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * Ho, 2 * Wo, C)


def pool_choice(act):
    """index in its 2x2 window of each window's first maximum in scan order (torch's max_pool2d rule): (B, H/2, W/2, C)"""
    return _windows(act).argmax(-1)


def max_pool(act):
    """the 2x2 / stride-2 max of act, in act's own type (exact)"""
    return _windows(act).amax(-1)


TAIL = namedtuple("TAIL", "out pool mean var var_unbiased dy dgamma dbeta")


def tail_node(y, gamma, beta, eps, act=None, dskip=None, dpool=None, running=None):
    """float64 encoder block tail: a = relu(bn(y)) (the skip), its 2x2 max-pool and the backward of dskip + the pooled gradient routed
    to each window's first maximum.  `act`: the device's stored activations -- the ReLU mask is act > 0 and the pool routing is decided
    on them; None: both decided on this reference's own values."""
    fwd = bn_node(y, gamma, beta, eps, mask=None if act is None else act > 0, running=running)
    dec = fwd.out if act is None else act
    choice = pool_choice(dec)
    pool = torch.gather(_windows(fwd.out), -1, choice.unsqueeze(-1)).squeeze(-1)
    dy = dgamma = dbeta = None
    if dskip is not None or dpool is not None:
        da = torch.zeros_like(fwd.out) if dskip is None else dskip.double()
        if dpool is not None:
            routed = torch.zeros(*choice.shape, 4, dtype=torch.float64, device=y.device)
            routed.scatter_(-1, choice.unsqueeze(-1), dpool.double().unsqueeze(-1))
            da = da + _unwindows(routed)
        b = bn_node(y, gamma, beta, eps, mask=fwd.mask, dout=da, running=running)
        dy, dgamma, dbeta = b.dy, b.dgamma, b.dbeta
    return TAIL(fwd.out, pool, fwd.mean, fwd.var, fwd.var_unbiased, dy, dgamma, dbeta)


def running_update(pre, bn: BN, momentum):
    """float64 running (mean, var) after one training-mode call of a BatchNorm2d whose running statistics were `pre` (the module)"""
    m = momentum
    return ((1 - m) * pre.running_mean.double() + m * bn.mean, (1 - m) * pre.running_var.double() + m * bn.var_unbiased)


# ------------------------------------------------------------------------------------------------ the recorder

# the blocks of mfai's UNet: (node-name prefix, attribute of the model, prefix of the Sequential's keys)
BLOCKS = [("enc1", "encoder1", "enc1"), ("enc2", "encoder2", "enc2"), ("enc3", "encoder3", "enc3"), ("enc4", "encoder4", "enc4"),
          ("bottleneck", "bottleneck", "bottleneck"), ("dec4", "decoder4", "dec4"), ("dec3", "decoder3", "dec3"),
          ("dec2", "decoder2", "dec2"), ("dec1", "decoder1", "dec1")]

# node kinds: "conv" (conv2d_nhwc), "bn" (batch_norm_act), "tail" (enc_tail), "up" (upconv_into)
COUNTS_NATIVE = {"conv": 19, "bn": 14, "tail": 4, "up": 4}
COUNTS_F32 = {"conv": 0, "bn": 14, "tail": 4, "up": 0}

# per kind: the Function's backward results that are gradients of the named inputs
GRAD_SLOTS = {"conv": {"x": 0, "w": 1, "b": 2}, "bn": {"y": 0, "gamma": 2, "beta": 3}, "tail": {"y": 0, "gamma": 2, "beta": 3},
              "up": {"x": 0, "w": 1, "b": 2, "buf": 3}}


def schedule(model):
    """[(kind, node name, module)] in the order UNetMI355X.forward calls its nodes (the bf16 route; fp32: the batch norms only)"""
    s = []
    for short, attr, key in BLOCKS:
        seq = getattr(model, attr)
        lvl = short[-1]
        if short.startswith("dec"):
            s.append(("up", f"upconv{lvl}", getattr(model, f"upconv{lvl}")))
        s += [("conv", f"{short}.conv1", seq[0]), ("bn", f"{short}.norm1", seq[1]), ("conv", f"{short}.conv2", seq[3])]
        s.append(("tail" if short.startswith("enc") else "bn", f"{short}.norm2", seq[4]))
    s.append(("conv", "head", model.conv))
    if not model.native:
        s = [e for e in s if e[0] in ("bn", "tail")]
    return s


def param_of(t):
    """the leaf parameter behind t: t itself, or the leaf a derived weight (F.pad of it) was made from"""
    if t is None or t.is_leaf:
        return t
    fn = t.grad_fn
    while fn is not None and not hasattr(fn, "variable"):
        fn = fn.next_functions[0][0] if fn.next_functions else None
    return None if fn is None else fn.variable


def _clone(t):
    return None if t is None else t.detach().clone()


def _key(t):
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()))


class Node:
    """one recorded call: kind, name, module (the live layer), pre (deep copy of its batch norm before the call), args (input clones),
    src (input name -> (node index, output index) of the recorded output it is), out (output clones), gout (the gradients the outputs
    received), gin (the Function's backward results), opts (the call's options); post: the batch norm right after the call"""

    def __init__(self, kind, name, module, args, opts):
        self.kind, self.name, self.module, self.args, self.opts = kind, name, module, args, opts
        self.pre = copy.deepcopy(module) if kind in ("bn", "tail") else None
        self.post = None
        self.src, self.out, self.gout, self.gin = {}, None, None, None

    def grad(self, slot):
        """the gradient this node's backward returned for input `slot`"""
        return self.gin[GRAD_SLOTS[self.kind][slot]]

    def params(self):
        """{slot: leaf parameter} of this node"""
        if self.kind in ("bn", "tail"):
            return {"gamma": self.module.weight, "beta": self.module.bias}
        ps = {"w": self.module.weight}
        if self.module.bias is not None:
            ps["b"] = self.module.bias
        return ps


class Recorder:
    """``with Recorder(model) as rec: y = model(x); y.backward(dy)`` -- rec.nodes in call order; the node counts are asserted on exit"""

    def __init__(self, model):
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
    def _begin(self, kind, module_arg, args, opts):
        i = len(self.nodes)
        assert i < len(self.expected), f"node {i} ({kind}): more node calls than UNetMI355X.forward makes ({len(self.expected)})"
        ekind, name, module = self.expected[i]
        assert kind == ekind, f"node {i}: expected {ekind} {name}, got a {kind} call"
        who = module if kind in ("bn", "tail") else param_of(module_arg)
        want = module if kind in ("bn", "tail") else module.weight
        assert who is want, f"{name}: the call's layer is not the model's {name}"
        node = Node(kind, name, module, {k: _clone(v) for k, v in args.items()}, opts)
        for k, v in args.items():
            if isinstance(v, torch.Tensor) and _key(v) in self._made:
                node.src[k] = self._made[_key(v)]
        return node

    def _end(self, node, outs, ctx):
        node.out = [_clone(o) for o in outs]
        if node.pre is not None:
            node.post = copy.deepcopy(node.module)
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
        from py4cast_amd import ops_gemm as G
        from py4cast_amd import unet as U

        rec = self
        conv0, bn0, tail0, up0 = G.conv2d_nhwc, G.batch_norm_act, U.enc_tail, U.upconv_into

        def conv2d_nhwc(x, w, b=None, res=None, want_stats=False, passthrough=False):
            assert res is None and not passthrough, "UNet's convolutions take no residual"
            node = rec._begin("conv", w, {"x": x, "w": w, "b": b}, {"want_stats": bool(want_stats)})
            out = conv0(x, w, b, res=res, want_stats=want_stats, passthrough=passthrough)
            y, st = out if want_stats else (out, None)
            rec._end(node, [y, st], y.grad_fn)
            return out

        def batch_norm_act(y, stats, bn, slope=1.0, **kw):
            assert not kw, "UNet's batch norms take no residual / multiplier"
            node = rec._begin("bn", bn, {"y": y, "stats": stats}, {"slope": float(slope)})
            out = bn0(y, stats, bn, slope=slope)
            rec._end(node, [out], out.grad_fn)
            return out

        def enc_tail(y, stats, bn):
            node = rec._begin("tail", bn, {"y": y, "stats": stats}, {})
            buf, pool = tail0(y, stats, bn)
            rec._end(node, [buf, pool], buf.grad_fn)
            return buf, pool

        def upconv_into(x, w, b, buf, grad_owned=False):
            node = rec._begin("up", w, {"x": x, "w": w, "b": b, "buf": buf}, {"grad_owned": bool(grad_owned)})
            out = up0(x, w, b, buf, grad_owned=grad_owned)
            rec._end(node, [out], out.grad_fn)
            return out

        self._mp = pytest.MonkeyPatch()
        self._mp.setattr(G, "conv2d_nhwc", conv2d_nhwc)
        self._mp.setattr(G, "batch_norm_act", batch_norm_act)
        self._mp.setattr(U, "enc_tail", enc_tail)
        self._mp.setattr(U, "upconv_into", upconv_into)
        for fn_cls in (G._Conv, G._BatchNormAct, U._EncTail, U._UpConvInto):
            self._wrap_backward(fn_cls)
        return self

    def __exit__(self, exc_type, exc, tb):
        self._mp.undo()
        self._keep = []
        if exc_type is None:
            want = COUNTS_NATIVE if self.model.native else COUNTS_F32
            got = {k: sum(n.kind == k for n in self.nodes) for k in want}
            assert got == want, f"UNet node calls {got}, expected {want}: a model change routes around the recorded entry points"
        return False
