"""
Node-level oracle of the native SwinUNETR (py4cast_amd/swinunetr.py): float64 references of the network's nodes, a recorder of the node
calls of a forward / backward, and the route table (which kernel serves which layer at which grid) -- the helpers of
tests/test_swin_nodes_gpu.py (the device) and tests/test_swin_nodes_cpu.py (the references themselves, against oracle/swinunetr.py and the
transformers goldens).

References: features-last float64 functions that run on CPU or GPU tensors alike and differentiate through torch autograd; `node()`
turns one into (outputs, gradients) for a recorded incoming gradient.  The attention and the Swin / merging algebra are
oracle/window_attention.py's and oracle/swinunetr.py's, the convolution is unet_nodes.conv.  Activations are taken as given (the recorded
bf16 tensors, promoted).  A weight is rounded to bf16 exactly where the kernel reads a bf16 image of it -- the GEMM and convolution
weights of the bf16 flavour (`gemm_w`); LayerNorm, instance-norm and bias parameters stay the fp32 values they are, and the relative
position table is gathered in fp32.  The fused MLP stores its hidden activation gelu(fc1 x) as bf16: `mlp(..., round_hidden=True)` rounds
it there (straight-through in the backward).  With rounding off everything is plain float64 (tests/test_swin_nodes_cpu.py).

Decisions: the only one is the LeakyReLU sign of the instance-norm node.  `inorm_act(..., sign_of=stored output)` takes it from the
device's stored output for a backward, so that no gradient comparison crosses a decision (as unetrpp_nodes.bn_act_node).
"""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from oracle import window_attention as owa

import unet_nodes as UN

# ------------------------------------------------------------------------------------------------ float64 node references


def gemm_w(w, on=True):
    """the weight as a bf16 GEMM / convolution reads it (on), as float64"""
    w = w.detach()
    return (w.to(torch.bfloat16) if on else w).double()


def round_bf16(t):
    """t rounded to bf16, straight-through for the gradient"""
    return t + (t.detach().to(torch.bfloat16).double() - t.detach())


def row_mask(B, Hp, Wp, H, W, device):
    """(B Hp Wp, 1) float64: 1 for the tokens inside (H, W), 0 for the padding tokens of a (B, Hp, Wp) map"""
    m = torch.zeros(B, Hp, Wp, 1, dtype=torch.float64, device=device)
    m[:, :H, :W] = 1
    return m.view(-1, 1)


def ln(x, g, b, eps=1e-5, mask=None):
    """row LayerNorm over the last dimension; mask = (Hp, Wp, H, W): x holds the rows of (B, Hp, Wp) maps whose tokens beyond (H, W) are
    padding -- their rows are zero forward, and take and give no gradient.  g = b = None: no affine (the hidden states)."""
    C = x.shape[-1]
    y = F.layer_norm(x, (C,), g, b, eps)
    if mask is not None:
        Hp, Wp, H, W = mask
        y = (y.reshape(-1, C) * row_mask(x.numel() // (C * Hp * Wp), Hp, Wp, H, W, x.device)).view(x.shape)
    return y


def attn_core(qkv, bias, heads, ws, shift):
    return owa.window_attention(qkv, bias, heads, ws, shift)


def table_rows(table, index):
    return table[index]


def table_rows_grad(index, rows, dy):
    """the gradient of table[index] for dy: dy's rows summed per table row (index_put_ with accumulate)"""
    return torch.zeros(rows, dy.shape[-1], dtype=dy.dtype, device=dy.device).index_put_((index,), dy, accumulate=True)


def linear(x, w, b=None, res=None):
    y = x @ w.t()
    if b is not None:
        y = y + b
    return y if res is None else y + res


def mlp(x, w1, b1, w2, b2, res, round_hidden=False):
    """res + fc2(gelu(fc1 x)); round_hidden: gelu(fc1 x) rounded to bf16, as the fused nodes store it"""
    h = F.gelu(linear(x, w1, b1))
    if round_hidden:
        h = round_bf16(h)
    return linear(h, w2, b2, res)


conv = UN.conv


def inorm_act(x, gamma, beta, eps=1e-5, slope=1.0, res=None, sign_of=None):
    """leaky_relu(IN(x) gamma + beta (+ res), slope), statistics over (H, W) per sample and channel (biased variance).  sign_of: a
    tensor whose sign decides the LeakyReLU branch instead of this reference's own pre-activation (the device's stored output)."""
    mean = x.mean(dim=(1, 2), keepdim=True)
    var = x.var(dim=(1, 2), unbiased=False, keepdim=True)
    z = (x - mean) * torch.rsqrt(var + eps) * gamma + beta
    if res is not None:
        z = z + res
    if slope == 1.0:
        return z
    pos = (z if sign_of is None else sign_of).detach() > 0
    return z * torch.where(pos, torch.ones_like(z), torch.full_like(z, float(slope)))


def upsample2(up, B, H, W, cout):
    """rows of (2, 2, cout) pixel blocks -> the (B, 2H, 2W, cout) grid (the transposed convolution's interleave)"""
    return up.view(B, H, W, 2, 2, cout).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, cout)


def transp_weight(wt):
    """ConvTranspose2d weight (cin, cout, 2, 2) -> the GEMM's (4 cout, cin) [dy][dx][cout] rows"""
    return wt.permute(2, 3, 1, 0).reshape(-1, wt.shape[0])


def merge_gather(x):
    """[x(0::2,0::2) | x(1::2,0::2) | x(0::2,1::2) | x(1::2,1::2)] along the channels, odd grids zero-padded at the bottom / right"""
    H, W = x.shape[1], x.shape[2]
    if H % 2 or W % 2:
        x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], dim=-1)


BLOCK_PARAMS = ("norm1.weight", "norm1.bias", "qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "relative_position_bias_table",
                "norm2.weight", "norm2.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
MERGE_PARAMS = ("norm.weight", "norm.bias", "reduction.weight")
GEMM_WEIGHTS = ("qkv.weight", "proj.weight", "fc1.weight", "fc2.weight", "reduction.weight")


def module_leaves(mod, names, rounded):
    """float64 leaves of a module's parameters as its nodes read them (GEMM weights bf16-rounded when `rounded`)"""
    ps = dict(mod.named_parameters())
    return {n: (gemm_w(ps[n], rounded) if n in GEMM_WEIGHTS else ps[n].detach().double()).requires_grad_(True) for n in names}


def block(x, P, heads, ws, shift, eps=1e-5, real=None, round_hidden=False):
    """SwinBlock.forward composed of the node references.  x (B, H, W, C), or with real = (H, W) the map padded to multiples of the
    window, which stays padded: norm1 zeroes the padding rows, everything after it is row-wise or the attention."""
    B, H, W, C = x.shape
    if real is not None:
        H, W = real
    shift = shift if min(H, W) > ws else 0
    mask = None if real is None else (x.shape[1], x.shape[2], H, W)
    h = ln(x, P["norm1.weight"], P["norm1.bias"], eps, mask)
    pb, pr = (0, 0) if real is not None else ((-H) % ws, (-W) % ws)
    if pb or pr:
        h = F.pad(h, (0, 0, 0, pr, 0, pb))
    N = ws * ws
    index = owa.relative_position_index(ws).view(-1).to(x.device)
    bias = table_rows(P["relative_position_bias_table"], index).view(N, N, heads).permute(2, 0, 1)
    a = attn_core(linear(h, P["qkv.weight"], P["qkv.bias"]), bias, heads, ws, shift)
    x = x + linear(a, P["proj.weight"], P["proj.bias"])[:, :x.shape[1], :x.shape[2], :]
    return mlp(ln(x, P["norm2.weight"], P["norm2.bias"], eps), P["fc1.weight"], P["fc1.bias"], P["fc2.weight"], P["fc2.bias"], x, round_hidden)


def merge(x, P, eps=1e-5):
    """PatchMerging.forward: gather, LayerNorm over 4 C, reduction to 2 C without bias"""
    return linear(ln(merge_gather(x), P["norm.weight"], P["norm.bias"], eps), P["reduction.weight"])


def res_block(x, P, pre, down, eps=1e-5):
    out = inorm_act(conv(x, P[pre + "conv1.weight"]), P[pre + "norm1.weight"], P[pre + "norm1.bias"], eps, 0.01)
    r = inorm_act(conv(x, P[pre + "conv3.weight"]), P[pre + "norm3.weight"], P[pre + "norm3.bias"], eps) if down else x
    return inorm_act(conv(out, P[pre + "conv2.weight"]), P[pre + "norm2.weight"], P[pre + "norm2.bias"], eps, 0.01, r)


def up_block(x, skip, P, pre):
    B, H, W, _ = x.shape
    wt = P[pre + "transp_conv.weight"]
    up = upsample2(linear(x.reshape(-1, x.shape[-1]), transp_weight(wt)), B, H, W, wt.shape[1])
    return res_block(torch.cat([up, skip], dim=-1), P, pre + "conv_block.", True)


def network(x, P, ws=7, depths=(2, 2, 2, 2), num_heads=(3, 6, 12, 24)):
    """the whole SwinUNETR forward composed of the node references above, on a dict P of float64 parameters under the model's names
    (no rounding anywhere): what tests/test_swin_nodes_cpu.py holds against oracle/swinunetr.py"""
    B, H, W, C = x.shape
    pw = P["patch_embed.weight"].permute(0, 2, 3, 1)                        # (fs, 2, 2, C)
    patches = x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4 * C)
    t = linear(patches, pw.reshape(pw.shape[0], -1), P["patch_embed.bias"])
    hidden = [ln(t, None, None)]
    for i, (depth, heads) in enumerate(zip(depths, num_heads)):
        h, w = t.shape[1], t.shape[2]
        pb, pr = (-h) % ws, (-w) % ws
        once = bool(pb or pr)                                               # padded once for the stage, as padded_stage does
        if once:
            t = F.pad(t, (0, 0, 0, pr, 0, pb))
        for j in range(depth):
            Pb = {n: P[f"stages.{i}.{j}.{n}"] for n in BLOCK_PARAMS}
            t = block(t, Pb, heads, ws, 0 if j % 2 == 0 else ws // 2, real=(h, w) if once else None)
        t = merge(t[:, :h, :w, :], {n: P[f"merges.{i}.{n}"] for n in MERGE_PARAMS})
        hidden.append(ln(t, None, None))
    fs = P["patch_embed.weight"].shape[0]
    enc0 = res_block(x, P, "encoder1.", x.shape[-1] != fs)
    enc1 = res_block(hidden[0], P, "encoder2.", False)
    enc2 = res_block(hidden[1], P, "encoder3.", False)
    enc3 = res_block(hidden[2], P, "encoder4.", False)
    dec4 = res_block(hidden[4], P, "encoder10.", False)
    dec3 = up_block(dec4, hidden[3], P, "decoder5.")
    dec2 = up_block(dec3, enc3, P, "decoder4.")
    dec1 = up_block(dec2, enc2, P, "decoder3.")
    dec0 = up_block(dec1, enc1, P, "decoder2.")
    out = up_block(dec0, enc0, P, "decoder1.")
    ow = P["out.weight"]
    return linear(out, ow.view(ow.shape[0], ow.shape[1]), P["out.bias"])


def leaf(t):
    return None if t is None else t.detach().double().requires_grad_(True)


def node(fn, inputs, dy):
    """fn(*inputs) on float64 leaves of `inputs` (None entries stay None, non-tensors pass through): (y, [gradients]) for dy"""
    leaves = [leaf(t) if isinstance(t, torch.Tensor) and t.is_floating_point() else t for t in inputs]
    with torch.enable_grad():
        y = fn(*leaves)
        live = [t for t in leaves if isinstance(t, torch.Tensor) and t.requires_grad]
        got = iter(torch.autograd.grad(y, live, dy.double(), allow_unused=True))
    return y.detach(), [next(got) if isinstance(t, torch.Tensor) and t.requires_grad else None for t in leaves]


# ------------------------------------------------------------------------------------------------ routes

LINEAR_ROUTES = ("row_gemm", "tiled_gemm", "library")
MLP_ROUTES = ("row_mlp", "tiled_mlp", "library")
CONV_ROUTES = ("conv_mfma", "conv_igemm", "conv_library")


def _w(shape):
    return torch.empty(shape, dtype=torch.float32)


def lin_route_rows(rows, O, K, has_bias, direct=False):
    """the route of a bf16 Linear over `rows` rows with an fp32 (O, K) weight, from swinunetr._lin's predicates; direct: a bare
    ops_rows.linear_nd call (the patch embedding, the output head: zero rows appended up to a multiple of 8 from 65 536 rows)"""
    from py4cast_amd import ops_rows as R

    b = _w((O,)) if has_bias else None
    if direct:
        if O % 8 and rows >= 65536:
            O8 = (O + 7) // 8 * 8
            if R._row_gemm_mode_rows(rows, _w((O8, K)), None if b is None else _w((O8,))) == "all":
                return "row_gemm"
        return "row_gemm" if R._row_gemm_mode_rows(rows, _w((O, K)), b) == "all" else "library"
    row = R._row_gemm_mode_rows(rows, _w((O, K)), b) == "all"
    if O % 8 == 0 and K % 8 == 0 and not row:
        return "tiled_gemm"
    return "row_gemm" if row else "library"


def mlp_route_rows(rows, dim, hidden):
    from py4cast_amd import ops_rows as R

    row1 = R._row_gemm_mode_rows(rows, _w((hidden, dim)), _w((hidden,))) == "all"
    if dim % 8 == 0 and hidden % 8 == 0 and not row1:
        return "tiled_mlp"
    if row1 and R._row_gemm_mode_rows(rows, _w((dim, hidden)), _w((dim,))) == "all":
        return "row_mlp"
    return "library"


def conv_route_channels(Co, Ci, Cx):
    """the route of a bias-free bf16 3x3 / 1x1 convolution (Co, Ci) on a map of Cx channels, from swinunetr._conv_hw's predicates"""
    if Co <= 64 and Ci <= 96:
        return "conv_mfma"
    if Co % 8 == 0 and Ci % 8 == 0 and Cx >= Ci and Cx % 8 == 0:
        return "conv_igemm"
    return "conv_library"


def route_table(B, H, W, cin=69, cout=60, fs=24, ws=7, depths=(2, 2, 2, 2)):
    """{layer: route} of the bf16 flavour at a (B, H, W) input, from shapes alone (the predicates read shapes and dtypes only)"""
    t = {}
    Cp = cin + cin % 2
    t["patch_embed"] = lin_route_rows(B * (H // 2) * (W // 2), fs, 4 * Cp, True, direct=True)
    h, w = H // 2, W // 2
    for i, depth in enumerate(depths):
        d = fs * 2 ** i
        rows = B * (h + (-h) % ws) * (w + (-w) % ws)          # (a stage that needs padding is padded once and stays padded)
        for j in range(depth):
            pre = f"stages.{i}.{j}."
            t[pre + "qkv"] = lin_route_rows(rows, 3 * d, d, True)
            t[pre + "proj"] = lin_route_rows(rows, d, d, True)
            t[pre + "mlp"] = mlp_route_rows(rows, d, 4 * d)
        h, w = (h + 1) // 2, (w + 1) // 2
        t[f"merges.{i}.reduction"] = lin_route_rows(B * h * w, 2 * d, 4 * d, False)
    for name, ci, co in (("encoder1", cin, fs), ("encoder2", fs, fs), ("encoder3", 2 * fs, 2 * fs), ("encoder4", 4 * fs, 4 * fs),
                         ("encoder10", 16 * fs, 16 * fs)):
        t.update(_res_routes(name + ".", ci, co, ci))
    for name, ci, co, lvl in (("decoder5", 16 * fs, 8 * fs, 5), ("decoder4", 8 * fs, 4 * fs, 4), ("decoder3", 4 * fs, 2 * fs, 3),
                              ("decoder2", 2 * fs, fs, 2), ("decoder1", fs, fs, 1)):
        t[name + ".transp_conv"] = lin_route_rows(B * (H >> lvl) * (W >> lvl), 4 * co, ci, False)
        t.update(_res_routes(name + ".conv_block.", 2 * co, co, 2 * co))
    t["out"] = lin_route_rows(B * H * W, cout, fs, True, direct=True)
    return t


def _res_routes(pre, ci, co, cx):
    t = {pre + "conv1": conv_route_channels(co, ci, cx), pre + "conv2": conv_route_channels(co, co, co)}
    if ci != co:
        t[pre + "conv3"] = conv_route_channels(co, ci, cx)
    return t


def smallest_grid_with_routes_of(B, H, W, **kw):
    """the smallest (by area, then height) grid of multiples of 32 whose route table is that of (H, W), and the table"""
    want = route_table(B, H, W, **kw)
    grids = sorted(((h, w) for h in range(32, H + 1, 32) for w in range(h, W + 1, 32)), key=lambda g: (g[0] * g[1], g[0]))
    for g in grids:
        if route_table(B, g[0], g[1], **kw) == want:
            return g, want
    return (H, W), want


# ------------------------------------------------------------------------------------------------ the recorder

KINDS = ("ln", "attn", "table", "linear", "mlp", "conv", "inorm", "block", "merge")
NODE_COUNTS = {"ln": 25, "attn": 8, "table": 8, "linear": 27, "mlp": 8, "conv": 26, "inorm": 26, "block": 8, "merge": 4}
NODE_COUNTS_F32 = dict(NODE_COUNTS, linear=22, ln=24)      # (there the five transposed convolutions are bare library matmuls and
#                                                               the 384-wide last hidden state takes the library LayerNorm)


def param_of(t):
    return UN.param_of(t)


class Node:
    """one recorded call: kind, name (the layer's name in the model), module (the live layer or None), args (operand clones), opts,
    route, out (clone of the output), dy (the gradient the output received), parent (index of the enclosing block / merge node),
    src ({operand: index of the node whose output it is})"""

    def __init__(self, kind, name, module, args, opts, route, parent):
        self.kind, self.name, self.module, self.args, self.opts, self.route, self.parent = kind, name, module, args, opts, route, parent
        self.out = self.dy = None
        self.src = {}


def _c(t):
    return None if t is None else t.detach().clone()


def _key(t):
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype)


class Recorder:
    """``with Recorder(model) as rec: model(x).backward(dy)``: rec.nodes in call order.  Wraps the module-level callables swinunetr.py
    calls (window_attention, _TableRows.apply, _layer_norm, _lin, _mlp, _conv_hw, _inorm; ops_rows.row_layer_norm and ops_rows.linear_nd
    where the model calls them directly: the hidden states, the patch embedding, the output head) and SwinBlock.forward /
    PatchMerging.forward.  The calls themselves are untouched: same arguments, same kernels."""

    def __init__(self, model):
        self.model = model
        self.nodes = []
        self.names = {id(m): n for n, m in model.named_modules()}
        self.pnames = {id(p): n for n, p in model.named_parameters()}
        self._depth = 0          # inside a recorded leaf call (its inner calls are its own business)
        self._stack = []         # enclosing block / merge nodes
        self._made = {}
        self._hidden = 0

    def __getitem__(self, name):
        got = [n for n in self.nodes if n.name == name]
        assert len(got) == 1, (name, len(got))
        return got[0]

    def of(self, *kinds):
        return [n for n in self.nodes if n.kind in kinds]

    # -------------------------------------------------------------- bookkeeping
    def _begin(self, kind, name, module, args, opts, route):
        node = Node(kind, name, module, {k: _c(v) if isinstance(v, torch.Tensor) else v for k, v in args.items()}, opts, route,
                    self._stack[-1] if self._stack else None)
        for k, v in args.items():
            if isinstance(v, torch.Tensor) and _key(v) in self._made:
                node.src[k] = self._made[_key(v)]
        return node

    def _end(self, node, out):
        node.out = _c(out)
        if out.requires_grad:
            out.register_hook(lambda g: setattr(node, "dy", g.detach().clone()))
        self.nodes.append(node)
        self._made[_key(out)] = len(self.nodes) - 1
        node.index = len(self.nodes) - 1
        self._keep.append(out)       # (keeps the storage alive: a recycled address must not be taken for this output)
        return out

    def _leaf_call(self, orig, *a, **kw):
        """run a leaf callable with nested recording off"""
        self._depth += 1
        try:
            return orig(*a, **kw)
        finally:
            self._depth -= 1

    def _wname(self, w):
        p = param_of(w)
        return self.pnames[id(p)].rsplit(".", 1)[0]

    # -------------------------------------------------------------- routes, from the predicates the model evaluates
    def _lin_route(self, x, w, b, direct):
        from py4cast_amd import ops_gemm as G
        from py4cast_amd import ops_rows as R
        from py4cast_amd import swinunetr as S

        if direct:
            O = w.shape[0]
            if O % 8 and w.dim() == 2 and x.is_cuda and x.numel() // max(w.shape[1], 1) >= 65536:
                O8 = (O + 7) // 8 * 8
                if R._row_gemm_mode(x, F.pad(w, (0, 0, 0, O8 - O)), None if b is None else F.pad(b, (0, O8 - O))) == "all":
                    return "row_gemm"
            return "row_gemm" if R._row_gemm_mode(x, w, b) == "all" else "library"
        if S._native(x) and G.supported(x, w) and not R._row_gemm_ok(x, w, b):
            return "tiled_gemm"
        return "row_gemm" if R._row_gemm_ok(x, w, b) else "library"

    def _mlp_route(self, fc1, fc2, x):
        from py4cast_amd import ops_gemm as G
        from py4cast_amd import ops_rows as R
        from py4cast_amd import swinunetr as S

        if S._native(x) and G.supported(x, fc1.weight) and G.supported(x, fc2.weight) and not R._row_gemm_ok(x, fc1.weight, fc1.bias):
            return "tiled_mlp"
        if S._native(x) and R.row_mlp_gelu_ok(x, fc1.weight, fc1.bias, fc2.weight, fc2.bias):
            return "row_mlp"
        return "library"

    def _conv_route(self, m, x):
        from py4cast_amd import ops_gemm as G
        from py4cast_amd import ops_model as OM
        from py4cast_amd import swinunetr as S

        if OM.conv_nhwc_supported(x, m.weight):
            return "conv_mfma"
        if (S._native(x) and m.bias is None and G.conv_supported(x, m.weight) and m.kernel_size[0] in (1, 3)
                and m.padding == (m.kernel_size[0] // 2,) * 2):
            return "conv_igemm"
        return "conv_library"

    # -------------------------------------------------------------- the wrappers
    def __enter__(self):
        from py4cast_amd import ops_rows as R
        from py4cast_amd import swinunetr as S

        rec, self._keep = self, []
        o = SimpleNamespace(attn=S.window_attention, table=S._TableRows.apply, ln=S._layer_norm, rln=R.row_layer_norm, lin=S._lin,
                            lnd=R.linear_nd, mlp=S._mlp, conv=S._conv_hw, inorm=S._inorm, block=S.SwinBlock.forward,
                            merge=S.PatchMerging.forward)
        self.orig = o

        def window_attention(qkv, bias, heads, ws, shift=0, scale=None):
            blk = rec.nodes[rec._stack[-1]]
            node = rec._begin("attn", blk.name + ".attn", None, {"qkv": qkv, "bias": bias}, {"heads": heads, "ws": ws, "shift": shift}, "native")
            return rec._end(node, rec._leaf_call(o.attn, qkv, bias, heads, ws, shift, scale))

        def table_apply(table, index, rows_of):
            node = rec._begin("table", rec.pnames[id(table)], None, {"table": table, "index": index, "rows_of": rows_of}, {}, "native")
            return rec._end(node, rec._leaf_call(o.table, table, index, rows_of))

        def _layer_norm(m, x, real=None):
            route = "native" if S._row_ln_ok(x) else "library"
            node = rec._begin("ln", rec.names[id(m)], m, {"x": x, "g": m.weight, "b": m.bias}, {"real": real, "eps": m.eps}, route)
            return rec._end(node, rec._leaf_call(o.ln, m, x, real))

        def row_layer_norm(x, gamma, beta, eps=1e-5, res=None, mask=None):
            if rec._depth:
                return o.rln(x, gamma, beta, eps, res, mask)
            assert res is None and mask is None and not gamma.requires_grad, "a bare row_layer_norm call that is not _hidden's"
            node = rec._begin("ln", f"hidden.{rec._hidden}", None, {"x": x, "g": gamma, "b": beta}, {"real": None, "eps": eps, "unit": True}, "native")
            rec._hidden += 1
            return rec._end(node, rec._leaf_call(o.rln, x, gamma, beta, eps, res, mask))

        def _lin(x, w, b=None, res=None):
            if rec._depth:
                return o.lin(x, w, b, res)
            node = rec._begin("linear", rec._wname(w), None, {"x": x, "w": w, "b": b, "res": res}, {"direct": False}, rec._lin_route(x, w, b, False))
            return rec._end(node, rec._leaf_call(o.lin, x, w, b, res))

        def linear_nd(x, w, b=None):
            if rec._depth:
                return o.lnd(x, w, b)
            node = rec._begin("linear", rec._wname(w), None, {"x": x, "w": w, "b": b, "res": None}, {"direct": True}, rec._lin_route(x, w, b, True))
            return rec._end(node, rec._leaf_call(o.lnd, x, w, b))

        def _mlp(fc1, fc2, x, res):
            name = rec.names[id(fc1)].rsplit(".", 1)[0] + ".mlp"
            node = rec._begin("mlp", name, (fc1, fc2), {"x": x, "res": res, "w1": fc1.weight, "b1": fc1.bias, "w2": fc2.weight, "b2": fc2.bias}, {},
                              rec._mlp_route(fc1, fc2, x))
            return rec._end(node, rec._leaf_call(o.mlp, fc1, fc2, x, res))

        def _conv_hw(m, x):
            node = rec._begin("conv", rec.names[id(m)], m, {"x": x, "w": m.weight}, {}, rec._conv_route(m, x))
            return rec._end(node, rec._leaf_call(o.conv, m, x))

        def _inorm(m, x, slope=1.0, res=None):
            node = rec._begin("inorm", rec.names[id(m)], m, {"x": x, "g": m.weight, "b": m.bias, "res": res}, {"slope": float(slope), "eps": m.eps}, "native")
            return rec._end(node, rec._leaf_call(o.inorm, m, x, slope, res))

        def composite(kind, orig):
            def forward(mod, x, *a, **kw):
                real = kw.get("real", a[0] if a else None)
                node = rec._begin(kind, rec.names[id(mod)], mod, {"x": x}, {"real": real}, None)
                node.index = len(rec.nodes)
                rec.nodes.append(node)               # (takes its place in call order before its inner nodes)
                rec._stack.append(node.index)
                try:
                    y = orig(mod, x, *a, **kw)
                finally:
                    rec._stack.pop()
                node.out = _c(y)
                y.register_hook(lambda g: setattr(node, "dy", g.detach().clone()))
                rec._made[_key(y)] = node.index      # (a composite's output is its last inner node's: the composite wins the edge)
                rec._keep.append(y)
                return y
            return forward

        self._mp = mp = pytest.MonkeyPatch()
        mp.setattr(S, "window_attention", window_attention)
        mp.setattr(S._TableRows, "apply", staticmethod(table_apply))
        mp.setattr(S, "_layer_norm", _layer_norm)
        mp.setattr(R, "row_layer_norm", row_layer_norm)
        mp.setattr(S, "_lin", _lin)
        mp.setattr(R, "linear_nd", linear_nd)
        mp.setattr(S, "_mlp", _mlp)
        mp.setattr(S, "_conv_hw", _conv_hw)
        mp.setattr(S, "_inorm", _inorm)
        mp.setattr(S.SwinBlock, "forward", composite("block", o.block))
        mp.setattr(S.PatchMerging, "forward", composite("merge", o.merge))
        return self

    def undo(self):
        self._mp.undo()
        self._keep = []

    def __exit__(self, exc_type, exc, tb):
        self.undo()
        if exc_type is None:
            want = NODE_COUNTS if self.model._settings.activation_dtype == "bf16" else NODE_COUNTS_F32
            got = {k: len(self.of(k)) for k in KINDS}
            assert got == want, f"SwinUNETR node calls {got}, expected {want}: a model change routes around the recorded entry points"
        return False
