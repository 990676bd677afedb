"""
Node-level oracle of the native Segformer (py4cast_amd/segformer.py): float64 references of the network's nodes and a recorder of the
node calls of a forward / backward -- the helpers of tests/test_segformer_nodes_gpu.py (the device) and tests/test_segformer_nodes_cpu.py
(the references themselves, against the modules of tests/segformer_reference.py).

Nodes: the channel LayerNorm, the spatial-reduction attention core softmax(q k^T scale) v, and the two PreNorm blocks as the model wires
them -- attention block x + to_out(SRA(to_q(LN x), to_kv(LN x))) and Mix-FFN block x + fc2(gelu(pw(dw3x3(fc1(LN x))))).
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


class Recorder:
    """wraps a SegformerMI355X's block methods (_attn, _ff) and the module-level chan_layer_norm / sr_attention the blocks call: per
    call, clones of the inputs and outputs, and for the blocks the gradient the output receives in the backward.  The calls themselves
    are untouched: same arguments, same kernels.  ``undo()`` restores everything."""

    def __init__(self, model):
        from py4cast_amd import segformer as S

        self.S, self.model = S, model
        self.blocks, self.norms, self.attns = [], [], []
        self.orig = {"_attn": model._attn, "_ff": model._ff, "chan_layer_norm": S.chan_layer_norm, "sr_attention": S.sr_attention}
        for kind in ("_attn", "_ff"):
            setattr(model, kind, self._block(kind, self.orig[kind]))
        S.chan_layer_norm = self._norm
        S.sr_attention = self._sra

    def _block(self, kind, orig):
        def run(pn, x):
            y = orig(pn, x)
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

    def undo(self):
        self.model._attn, self.model._ff = self.orig["_attn"], self.orig["_ff"]
        self.S.chan_layer_norm, self.S.sr_attention = self.orig["chan_layer_norm"], self.orig["sr_attention"]
