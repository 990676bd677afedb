"""
Node-level oracle of the native Segformer (py4cast_amd/segformer.py): float64 references of the network's nodes and a recorder of the
node calls of a forward / backward -- the helpers of tests/test_segformer_nodes_gpu.py (the device) and tests/test_segformer_nodes_cpu.py
(the references themselves, against the modules of tests/segformer_reference.py).

Nodes: the channel LayerNorm, the spatial-reduction attention core softmax(q k^T scale) v, and the two PreNorm blocks as the model wires
them -- attention block x + to_out(SRA(to_q(LN x), to_kv(LN x))) and Mix-FFN block x + fc2(gelu(pw(dw3x3(fc1(LN x))))).
Outside the blocks: the strided convolutions (downsampler, patch embeddings) as F.conv2d, the decoder's and the head's 1x1 convolutions as
F.linear, the decoder's nearest up-sampling sum, the final bilinear x8, and the decoder as the network states it (up-sample, concatenate,
one Conv2d(4 decoder_dim, decoder_dim, 1)) next to the per-stage column blocks the native route applies.
Features-last (B, H, W, C) float64 throughout; every function runs on CPU or GPU tensors alike.  The GEMM weights are taken rounded to
bf16 (the GEMM reads bf16 images of the fp32 parameters); the LayerNorm and depthwise parameters as given (those kernels read fp32).
"""
import torch
import torch.nn.functional as F


def ln(x, g, b, eps=1e-5):
    """lucidrains' LayerNorm over the last dimension: (x - mean) / (std_biased + eps) g + b"""
    C = x.shape[-1]
    sd = x.var(-1, unbiased=False, keepdim=True).sqrt()
    return (x - x.mean(-1, keepdim=True)) / (sd + eps) * g.reshape(C) + b.reshape(C)


def sra_core(q, kv, heads, scale):
    """q (B, Nq, D), kv (B, Nk, 2 D) (keys first) -> (B, Nq, D): per head softmax(q k^T scale) v"""
    B, Nq, D = q.shape
    Nk, dh = kv.shape[1], D // heads
    qh = q.reshape(B, Nq, heads, dh).transpose(1, 2)
    kh = kv[..., :D].reshape(B, Nk, heads, dh).transpose(1, 2)
    vh = kv[..., D:].reshape(B, Nk, heads, dh).transpose(1, 2)
    o = ((qh @ kh.transpose(-1, -2)) * scale).softmax(-1) @ vh
    return o.transpose(1, 2).reshape(B, Nq, D)


def _lin(x, w, b=None):
    y = x @ w.reshape(w.shape[0], -1).t()
    return y if b is None else y + b


def attn_block(x, g, b, eps, wq, wkv, wout, heads, r, scale):
    B, H, W, D = x.shape
    xn = ln(x, g, b, eps)
    q = _lin(xn, wq)
    kv = F.conv2d(xn.permute(0, 3, 1, 2), wkv, stride=r).permute(0, 2, 3, 1)
    o = sra_core(q.reshape(B, H * W, D), kv.reshape(B, -1, 2 * D), heads, scale)
    return _lin(o.reshape(B, H, W, D), wout) + x


def ff_block(x, g, b, eps, w1, b1, wdw, bdw, wpw, bpw, w2, b2):
    xn = ln(x, g, b, eps)
    h1 = _lin(xn, w1, b1)
    h2 = F.conv2d(h1.permute(0, 3, 1, 2), wdw, bdw, padding=1, groups=h1.shape[-1]).permute(0, 2, 3, 1)
    return _lin(F.gelu(_lin(h2, wpw, bpw)), w2, b2) + x


def patch_conv_ref(x, w2d, b, k, stride, pad):
    """Conv2d(C, D, k, stride, pad) of a features-last map, the weight as its (D, C k^2) view (nn.Unfold's column order c k^2 + ky k + kx)"""
    C = x.shape[-1]
    return F.conv2d(x.permute(0, 3, 1, 2), w2d.reshape(w2d.shape[0], C, k, k), b, stride=stride, padding=pad).permute(0, 2, 3, 1)


def linear_ref(x, w, b=None):
    return F.linear(x, w, b)


def up_sum_ref(z0, z1, z2, z3):
    """z0 + nearest x2 (z1) + nearest x4 (z2) + nearest x8 (z3)"""
    return sum(F.interpolate(z.permute(0, 3, 1, 2), scale_factor=2 ** i, mode="nearest").permute(0, 2, 3, 1) for i, z in enumerate((z0, z1, z2, z3)))


def upsample8_ref(x):
    return F.interpolate(x.permute(0, 3, 1, 2), scale_factor=8, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


def decoder_cat_ref(fused, w0, b0):
    """the decoder as the network states it: Conv2d(4 dd, dd, 1) (weight (dd, 4 dd[, 1, 1]), bias (dd)) of the concatenated stage maps
    ``fused[i]`` (B, H / 2^i, W / 2^i, dd), each up-sampled (nearest) to the first one's grid"""
    ups = [F.interpolate(f.permute(0, 3, 1, 2), scale_factor=2 ** i, mode="nearest") for i, f in enumerate(fused)]
    dd = w0.shape[0]
    return F.conv2d(torch.cat(ups, dim=1), w0.reshape(dd, -1, 1, 1), b0).permute(0, 2, 3, 1)


def decoder_sliced_ref(fused, w0, b0):
    """the same map as the native route computes it: stage i through columns [i dd, (i + 1) dd) of the weight at the stage's own
    resolution, the bias once (stage 0), then the nearest up-sampling sum"""
    dd = w0.shape[0]
    w = w0.reshape(dd, -1)
    return up_sum_ref(*[linear_ref(f, w[:, i * dd: (i + 1) * dd], b0 if i == 0 else None) for i, f in enumerate(fused)])


def _gemm_w(w):
    return w.detach().to(torch.bfloat16).double()


def _p(t):
    return t.detach().double()


def block_params(kind, pn):
    """(names, float64 leaves) of a PreNorm block's parameters as the native node reads them"""
    if kind == "attn":
        a = pn.fn
        named = [("norm.g", _p(pn.norm.g)), ("norm.b", _p(pn.norm.b)), ("fn.to_q.weight", _gemm_w(a.to_q.weight)),
                 ("fn.to_kv.weight", _gemm_w(a.to_kv.weight)), ("fn.to_out.weight", _gemm_w(a.to_out.weight))]
    else:
        fc1, ds, _, fc2 = pn.fn.net
        dw, pw = ds.net
        named = [("norm.g", _p(pn.norm.g)), ("norm.b", _p(pn.norm.b)), ("fn.net.0.weight", _gemm_w(fc1.weight)), ("fn.net.0.bias", _p(fc1.bias)),
                 ("fn.net.1.net.0.weight", _p(dw.weight)), ("fn.net.1.net.0.bias", _p(dw.bias)), ("fn.net.1.net.1.weight", _gemm_w(pw.weight)),
                 ("fn.net.1.net.1.bias", _p(pw.bias)), ("fn.net.3.weight", _gemm_w(fc2.weight)), ("fn.net.3.bias", _p(fc2.bias))]
    return [n for n, _ in named], [t.requires_grad_(True) for _, t in named]


def block_ref(kind, pn, x, leaves):
    """the float64 block node on x with the parameter leaves of block_params"""
    if kind == "attn":
        g, b, wq, wkv, wout = leaves
        a = pn.fn
        return attn_block(x, g, b, pn.norm.eps, wq, wkv, wout, a.heads, a.reduction_ratio, a.scale)
    return ff_block(x, leaves[0], leaves[1], pn.norm.eps, *leaves[2:])


class _ModuleProxy:
    """a module with some attributes overridden; everything else is the module's own"""

    def __init__(self, real, **over):
        self.__dict__.update(over)
        self.__dict__["_real"] = real

    def __getattr__(self, name):
        return getattr(self._real, name)


class Recorder:
    """wraps a SegformerMI355X's block methods (_attn, _ff) and the module-level names of py4cast_amd.segformer that _forward_native and
    the blocks call: chan_layer_norm, sr_attention, patch_conv, up_sum and (through a proxy of the module-level ``G``) G.linear and
    G.upsample_add.  Per call, clones of the inputs and outputs, and -- for the blocks and the nodes outside them -- the gradient the
    output receives in the backward.  The calls themselves are untouched: same arguments, same kernels.  ``undo()`` restores everything.

    blocks / norms / attns: as before (every block, every LayerNorm, every attention core).  Calls made OUTSIDE a block, in call order:
    ``patch_convs`` (the downsampler with its zero-padded input channels and padded weight, then the four embeddings), ``linears`` (the
    four decoder pairs to_fused[i] / to_segmentation.0's column block i, then the head), ``up_sums`` and ``upsamples`` (the head's x8,
    before the channel crop).  The blocks' own patch_conv (to_kv) / G.linear calls belong to the block nodes and are not listed."""

    def __init__(self, model):
        from py4cast_amd import segformer as S

        self.S, self.model = S, model
        self.blocks, self.norms, self.attns = [], [], []
        self.patch_convs, self.linears, self.up_sums, self.upsamples = [], [], [], []
        self.in_block = 0
        self.orig = {"_attn": model._attn, "_ff": model._ff, "chan_layer_norm": S.chan_layer_norm, "sr_attention": S.sr_attention,
                     "patch_conv": S.patch_conv, "up_sum": S.up_sum, "G": S.G}
        for kind in ("_attn", "_ff"):
            setattr(model, kind, self._block(kind, self.orig[kind]))
        S.chan_layer_norm = self._norm
        S.sr_attention = self._sra
        S.patch_conv = self._patch_conv
        S.up_sum = self._up_sum
        S.G = _ModuleProxy(S.G, linear=self._linear, upsample_add=self._upsample_add)

    @staticmethod
    def _c(t):
        return None if t is None else t.detach().clone()

    def _with_dy(self, rec, y):
        rec.update(y=y.detach().clone(), dy=None)
        if y.requires_grad:
            y.register_hook(lambda g: rec.__setitem__("dy", g.detach().clone()))
        return rec

    def _block(self, kind, orig):
        def run(pn, x):
            self.in_block += 1
            try:
                y = orig(pn, x)
            finally:
                self.in_block -= 1
            rec = {"kind": kind.strip("_"), "pn": pn, "x": x.detach().clone(), "y": y.detach().clone(), "dy": None}
            if y.requires_grad:
                y.register_hook(lambda g: rec.__setitem__("dy", g.detach().clone()))
            self.blocks.append(rec)
            return y
        return run

    def _norm(self, x, g, b, eps=1e-5, passthrough=False):
        out = self.orig["chan_layer_norm"](x, g, b, eps, passthrough)
        y = out[0] if passthrough else out
        self.norms.append({"x": x.detach().clone(), "g": g.detach().clone(), "b": b.detach().clone(), "eps": eps, "y": y.detach().clone()})
        return out

    def _sra(self, q, kv, heads, scale):
        out = self.orig["sr_attention"](q, kv, heads, scale)
        self.attns.append({"q": q.detach().clone(), "kv": kv.detach().clone(), "heads": heads, "scale": scale, "y": out.detach().clone()})
        return out

    def _patch_conv(self, x, w2d, b, k, stride, pad):
        y = self.orig["patch_conv"](x, w2d, b, k, stride, pad)
        if not self.in_block:
            self.patch_convs.append(self._with_dy({"x": self._c(x), "w": self._c(w2d), "b": self._c(b), "k": k, "stride": stride, "pad": pad}, y))
        return y

    def _linear(self, x, w, b=None, res=None):
        y = self.orig["G"].linear(x, w, b, res)
        if not self.in_block:
            self.linears.append(self._with_dy({"x": self._c(x), "w": self._c(w), "b": self._c(b), "res": self._c(res)}, y))
        return y

    def _up_sum(self, z0, z1, z2, z3):
        y = self.orig["up_sum"](z0, z1, z2, z3)
        self.up_sums.append(self._with_dy({"z": [self._c(z) for z in (z0, z1, z2, z3)]}, y))
        return y

    def _upsample_add(self, x, skip, scale):
        y = self.orig["G"].upsample_add(x, skip, scale)
        self.upsamples.append(self._with_dy({"x": self._c(x), "skip": self._c(skip), "scale": scale}, y))
        return y

    def undo(self):
        self.model._attn, self.model._ff = self.orig["_attn"], self.orig["_ff"]
        S = self.S
        S.chan_layer_norm, S.sr_attention = self.orig["chan_layer_norm"], self.orig["sr_attention"]
        S.patch_conv, S.up_sum, S.G = self.orig["patch_conv"], self.orig["up_sum"], self.orig["G"]
