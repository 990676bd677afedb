"""
SwinUNETR (py4cast_amd/swinunetr.py) node by node: one forward / backward of SwinUNetRMI355X (69 -> 60 channels, the benchmark's) under
tests/swin_nodes.py's recorder, then for every recorded node -- the row LayerNorms (plain, masked, unit-affine), the window attention
cores, the relative-position gathers, the Linears (row GEMM, tiled GEMM, library; patch embedding, transposed-convolution GEMMs and output
head included), the fused MLPs, the convolutions, the instance-norm nodes, and the composed SwinBlock / PatchMerging calls:

* replay: the node alone on its recorded operands and incoming gradient, with fresh parameter leaves, gives the in-network output BIT FOR
  BIT, and replayed twice the same gradients bit for bit (every native reduction has a fixed order).  Exempt: nodes whose route is
  `library` / `conv_library` and the composed nodes that contain one.  bf16: at 64 x 96 (toy-ws7, toy-ws8) the patch embedding and the
  output head, at every grid the 768-wide LayerNorm of the last merging (and so merges.3), nothing else; fp32 flavour: every Linear and
  MLP (and so every block and merging), the 384- and 768-wide LayerNorms of merges.2 / merges.3, the ten convolutions of encoder4,
  encoder10, decoder5 and decoder4 -- its attention, table, LayerNorm, instance-norm and 16 narrow convolution nodes are held bit for bit;
* float64: the replay against the node reference on the same operands.  Single-kernel nodes at the project's bars: bf16 maps <= 6e-3 of
  the largest magnitude per element and <= 3e-3 in the 2-norm; GEMM / convolution weight and bias gradients <= 5e-4 -- with ONE
  departure: the library route of a bf16 Linear hands its weight and bias gradient back ROUNDED TO bf16 (2^-9 per element, about 1.1e-3 in
  the 2-norm: above 5e-4 by the number format alone), so those are held to the bf16-map bars, the project's bar for a bf16-stored value.
  That is patch_embed and out in toy-ws7-bf16 and toy-ws8-bf16 (worst 2.0e-3 in the 2-norm) and no node of mid-bf16 / routes-bf16, where
  both run on the row GEMM and meet 5e-4; LayerNorm gamma / beta gradients <= 2e-3; attention core forward
  <= 6e-3, dqkv and dbias <= 1.5e-2, each of dq / dk / dv <= 2e-2; instance-norm node <= 1.5e-2 with the LeakyReLU sign of the backward
  taken from the stored output; the relative-position gather exact forward and <= 1e-5 backward (<= 49 fp32 additions per table row);
  fp32 flavour: outputs <= 1e-5, gradients <= 1e-4, the exact attention <= 2e-6 forward and <= 5e-6 backward.
  Composed nodes (mlp, block, merge: several bf16-stored intermediates, not all modelled) at no more than twice the worst measured value,
  COMPOSED_BARS below; the block's own part (y - x, dx - dy) is checked apart from the residual and must be >= 5 % of x;
* routes: the recorded route of every layer equals swin_nodes.route_table's (from shapes alone), and the `routes` case runs on the smallest
  grid of multiples of 32 whose table is that of 2 x 512 x 512;
* wiring: the gradient each node's output received is, bit for bit, what the replays of its consumers produced, over the whole graph.
  Swin half: attention dqkv -> qkv Linear, dbias -> the table gather through the (N, N, heads) view, qkv dx -> norm1, proj dx ->
  attention, norm2 dx + the MLP's residual gradient -> proj, MLP dx -> norm2, norm1 dx + proj's residual gradient = the block's dx, block
  to block along a stage, the stage's crop into the merging, reduction dx -> the merging's norm.  Decoder, from the head down: out dx ->
  decoder1, inside every ResBlock norm2 dx -> conv2 dx -> norm1 dx -> conv1 and norm2's residual gradient -> norm3 dx -> conv3 (the skip
  junction), conv1 dx + conv3 dx = the gradient of cat([up, skip]), its first channels through the 2 x 2 interleave -> the transposed
  convolution's GEMM, whose dx -> the block below, its last channels -> the encoder block / hidden state on the skip.  Hidden states: the
  decoder's gradient (conv1 dx + the residual's, or the cat slice) -> hidden.k, and hidden.k dx + the cropped dx of stage k's first block
  -> the patch embedding / merging k - 1.  Input: the network's dx is encoder1's conv1 dx + conv3 dx + the patch embedding's dx through
  the patch view (three terms: one of the three pairings).  An edge whose producer runs on a library route is held to 1e-2 (bf16) / 1e-5
  (fp32) instead; in the fp32 flavour the transposed convolutions and hidden.4 are no nodes and are recomputed with torch.
  The network's p.grad is the node replays' parameter gradient (through the patch / transposed-convolution /
  head weight layouts) and every parameter belongs to exactly one leaf node;
* sink route (bf16, toy-ws7): every .grad pre-filled, then under FlatDDP with a non-zero flat buffer: p.grad = prefill + the gradient of the
  .grad-is-None run, bit for bit.  The tiled GEMM's Linears / MLPs and the implicit-GEMM convolutions add into .grad in place; everything
  else (row-GEMM Linears, LayerNorm / instance-norm affine, tables, the permuted / zero-padded patch, transposed-convolution and head
  weights) goes through autograd's own accumulation.

Counts asserted: 140 nodes (25 LayerNorm, 8 attention, 8 table, 27 Linear, 8 MLP, 26 convolution, 26 instance norm, 8 block, 4 merging);
203 parameters, each owned by one leaf node.  fp32 flavour, as run: 134 nodes (24 LayerNorm, 22 Linear), 198 parameters owned -- its five
transposed convolutions are bare library matmuls and its 384-wide last hidden state goes through the library's LayerNorm.

The `routes` case: 2 x 288 x 416, the smallest grid of multiples of 32 with the route table of 2 x 512 x 512, which is
row_gemm: patch_embed, qkv / proj of stages 0-1, proj of stage 2, merges.0.reduction, decoder2 / decoder1.transp_conv, out (zero rows to 64);
tiled_gemm: qkv of stages 2-3, proj of stage 3, merges.1-3.reduction, decoder5 / 4 / 3.transp_conv; row_mlp: stages 0-1; tiled_mlp: stages
2-3; conv_mfma: encoder1-3, decoder3 / 2 / 1 (16 convolutions); conv_igemm: encoder4, encoder10, decoder5 / 4 (10).  (At 64 x 96 twelve
layers take another route, at 256 x 320 the two proj of stage 2.)

Measured on one MI355X, worst node over the four bf16 cases / bar: bf16 maps 3.7e-3 / 6e-3 per element and 2.0e-3 / 3e-3 in the 2-norm;
GEMM / convolution dW, db 3.9e-7 / 5e-4; LayerNorm dgamma, dbeta 2.5e-7 / 2e-3; attention out 1.9e-3 / 6e-3, dqkv and dbias 2.6e-3 /
1.5e-2, dq / dk / dv 2.7e-3 / 2e-2; instance norm 1.7e-3 / 1.5e-2; table gradient 7.4e-8 / 1e-5.  Composed nodes (bar <= 2 x worst):
mlp y - res 7.4e-3 / 1.4e-2, dx 2.5e-3 / 4.9e-3, dW 5.2e-3 / 1.0e-2, db 3.7e-3 / 7.0e-3; block y 3.0e-3 / 5.9e-3, y - x 7.4e-3 / 1.4e-2,
dx 2.7e-3 / 5.4e-3, dx - dy 9.3e-3 / 1.8e-2, parameter gradients 9.6e-3 / 1.9e-2 (qkv.weight 7.4e-3 / 1.4e-2: Segformer's dS = P (dP - D)
cancellation does not bite here, every parameter meets 3e-2 and none needs a cosine bar); merge y 2.4e-3 / 4.8e-3, dx 2.4e-3 / 4.7e-3,
parameter gradients 5.6e-3 / 1.1e-2; own part of every block and MLP >= 1.04 x the residual stream (bar 0.05).  fp32 flavour, worst of toy-ws7-f32 and mid-f32 / bar: outputs
6.3e-7 / 1e-5, gradients 4.2e-6 / 1e-4, composed outputs 5.8e-7 / 1e-5 and gradients 3.8e-6 / 1e-4, exact attention out 1.9e-7 / 2e-6,
dqkv and dbias 2.9e-7 / 5e-6, dq / dk / dv 1.2e-6 / 5e-6.  The whole file (30 tests) takes 11 s on one MI355X.
"""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import swin_nodes as N  # noqa: E402

pytestmark = pytest.mark.gpu

BENCH = (2, 512, 512)
# name -> (H, W) or None (the routes grid, searched), window, flavour
CASES = {
    "toy-ws7-bf16": ((64, 96), 7, "bf16"),        # every stage pads; stage 4 is <= the window: its shift is off
    "toy-ws8-bf16": ((64, 96), 8, "bf16"),        # window 8: stages 1-2 need no padding (the per-block route), 3-4 pad
    "mid-bf16": ((256, 320), 7, "bf16"),          # token grids 128 x 160 -> 133 x 161, 70 x 84, 35 x 42, 21 x 21: all pad and shift
    "routes-bf16": (None, 7, "bf16"),             # the smallest grid with the benchmark's routes
    "toy-ws7-f32": ((64, 96), 7, "f32"),          # the fp32 flavour: exact attention kernels, library GEMMs
    "mid-f32": ((256, 320), 7, "f32"),
}

# composed nodes: quantity -> bar (2-norm, relative); at most twice the worst measured value (MEASURED below)
COMPOSED_BARS = {
    "mlp y-res": 1.4e-2, "mlp dx": 4.9e-3, "mlp dW": 1.0e-2, "mlp db": 7.0e-3,
    "block y": 5.9e-3, "block y-x": 1.4e-2, "block dx": 5.4e-3, "block dx-dy": 1.8e-2, "block dparam": 1.9e-2, "block dqkv.weight": 1.4e-2,
    "merge y": 4.8e-3, "merge dx": 4.7e-3, "merge dparam": 1.1e-2,
}


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def same(got, want, what):
    assert got is not None and want is not None, f"{what}: missing ({got is None}, {want is None})"
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError(f"{what}: not bit-identical ({int((d > 0).sum())} elements differ, max {float(d.max()):.3e})")


class Tally:
    """collects every bar's worst value and every miss, so that one run reports them all"""

    def __init__(self, case):
        self.case, self.worst, self.missed = case, {}, []

    def bar(self, v, limit, what, key, lower=False):
        w = self.worst.get(key)
        if w is None or (v < w[0] if lower else v > w[0]):
            self.worst[key] = (v, limit, what)
        if limit is not None and ((v < limit) if lower else (v > limit)):
            self.missed.append(f"{what}: {v:.3e} {'<' if lower else '>'} {limit:.1e} [{key}]")

    def done(self):
        print(f"\n{self.case}: worst value / bar")
        for k, (v, lim, what) in sorted(self.worst.items()):
            print(f"    {k:28s} {v:.2e} / {'unset' if lim is None else format(lim, '.1e')}   ({what})")
        assert not self.missed, f"{self.case}: {len(self.missed)} misses:\n" + "\n".join(self.missed[:40])


def make_model(case, dev):
    from py4cast_amd.swinunetr import SwinUNetRMI355X, SwinUNetRSettings

    hw, ws, key = CASES[case]
    if hw is None:
        hw, _ = N.smallest_grid_with_routes_of(*BENCH)
    torch.manual_seed(51)
    m = SwinUNetRMI355X(69, 60, hw, SwinUNetRSettings(activation_dtype=key, window_size=ws)).to(dev)
    g = torch.Generator().manual_seed(52)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("relative_position_bias_table"):
                p.normal_(0, 0.5)
            elif "norm" in n:      # LayerNorm and instance-norm affine off their initial 1 / 0 by +-(0.1 ... 0.3): a dropped gamma / beta shows
                d = (0.1 + 0.2 * torch.rand(p.shape, generator=g)) * (1 - 2 * (torch.rand(p.shape, generator=g) < 0.5).float())
                p.add_(d.to(dev))
    gd = torch.Generator(device=dev).manual_seed(53)
    x = torch.randn(2, *hw, 69, device=dev, generator=gd)
    dy = torch.randn(2, *hw, 60, device=dev, generator=gd)
    return m, x, dy, hw


def step(m, x, dy):
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), xg.grad


@pytest.fixture(scope="module", params=list(CASES))
def run(request, gpu_device):
    torch.cuda.empty_cache()
    m, x, dy, hw = make_model(request.param, gpu_device)
    with N.Recorder(m) as rec:
        y, dx = step(m, x, dy)
    for n in rec.nodes:
        assert n.out is not None and n.dy is not None, f"{n.kind} {n.name}: no output / incoming gradient recorded"
    g_none = {name: p.grad.detach().clone() for name, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    yield SimpleNamespace(case=request.param, model=m, x=x, dy=dy, y=y, dx=dx, rec=rec, g_none=g_none, hw=hw, ws=CASES[request.param][1],
                          bf16=CASES[request.param][2] == "bf16", replays={})
    del m, rec, g_none
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ replay
def fresh(t):
    return None if t is None else t.detach().clone().requires_grad_(True)


def _replay(node):
    from py4cast_amd import ops_rows as R
    from py4cast_amd import swinunetr as S

    a, k, o = node.args, node.kind, node.opts
    if k in ("block", "merge"):
        mod = node.module
        for p in mod.parameters():
            p.grad = None
        x = fresh(a["x"])
        y = S.SwinBlock.forward(mod, x, real=o["real"]) if k == "block" else S.PatchMerging.forward(mod, x)
        y.backward(node.dy.clone())
        grads = {"x": x.grad, **{n: p.grad for n, p in mod.named_parameters()}}
        for p in mod.parameters():
            p.grad = None
        torch.cuda.synchronize()
        return SimpleNamespace(y=y.detach(), grads=grads)
    if k == "ln" and o.get("unit"):
        ins = {"x": fresh(a["x"])}
        y = R.row_layer_norm(ins["x"], a["g"], a["b"], o["eps"])
    elif k == "ln":
        ins = {s: fresh(a[s]) for s in ("x", "g", "b")}
        m = SimpleNamespace(weight=ins["g"], bias=ins["b"], eps=o["eps"], normalized_shape=(a["x"].shape[-1],))
        y = S._layer_norm(m, ins["x"], o["real"])
    elif k == "attn":
        ins = {s: fresh(a[s]) for s in ("qkv", "bias")}
        y = S.window_attention(ins["qkv"], ins["bias"], o["heads"], o["ws"], o["shift"])
    elif k == "table":
        ins = {"table": fresh(a["table"])}
        y = S._TableRows.apply(ins["table"], a["index"], a["rows_of"])
    elif k == "linear":
        ins = {s: fresh(a[s]) for s in ("x", "w", "b", "res")}
        y = R.linear_nd(ins["x"], ins["w"], ins["b"]) if o["direct"] else S._lin(ins["x"], ins["w"], ins["b"], ins["res"])
    elif k == "mlp":
        ins = {s: fresh(a[s]) for s in ("x", "res", "w1", "b1", "w2", "b2")}
        y = S._mlp(SimpleNamespace(weight=ins["w1"], bias=ins["b1"]), SimpleNamespace(weight=ins["w2"], bias=ins["b2"]), ins["x"], ins["res"])
    elif k == "conv":
        ins = {s: fresh(a[s]) for s in ("x", "w")}
        y = S._conv_hw(SimpleNamespace(weight=ins["w"], bias=None, kernel_size=node.module.kernel_size, padding=node.module.padding), ins["x"])
    else:
        ins = {s: fresh(a[s]) for s in ("x", "g", "b", "res")}
        y = S._inorm(SimpleNamespace(weight=ins["g"], bias=ins["b"], eps=o["eps"]), ins["x"], o["slope"], ins["res"])
    y.backward(node.dy.clone())
    torch.cuda.synchronize()
    return SimpleNamespace(y=y.detach(), grads={s: (None if t is None else t.grad) for s, t in ins.items()})


def replay(run, node):
    if node.index not in run.replays:
        run.replays[node.index] = _replay(node)
    return run.replays[node.index]


def from_library(run, node):
    """the node, or for a composed node one of its inner nodes, runs on a library route (no bit-for-bit promise)"""
    lib = ("library", "conv_library")
    return node.route in lib or any(n.parent == node.index and n.route in lib for n in run.rec.nodes)


def test_replay_is_bit_identical(run):
    exempt = []
    for node in run.rec.nodes:
        r = replay(run, node)
        what = f"{node.kind} {node.name} [{node.route}]"
        if from_library(run, node):
            exempt.append(what)
            assert rel(r.y, node.out) <= 1e-2, f"{what}: replayed output {rel(r.y, node.out):.2e} off the in-network one"
            continue
        same(r.y, node.out, f"{what} out")
        again = _replay(node)
        for s, g in r.grads.items():
            if g is not None or again.grads[s] is not None:
                same(again.grads[s], g, f"{what} d{s}, replayed twice")
    print(f"\n{run.case}: {len(run.rec.nodes)} nodes replayed; exempt from bit-identity (library routes): {exempt}")


# ------------------------------------------------------------------------------------------------ routes
def test_routes(run):
    """the recorded route of every layer is the one swin_nodes.route_table derives from the shapes; the `routes` case IS the benchmark's
    table, so a later change of a route predicate cannot silently un-cover a kernel"""
    rec = run.rec
    got = {n.name: n.route for n in rec.of("linear", "mlp", "conv")}
    if not run.bf16:
        assert set(got.values()) <= {"library", "conv_mfma", "conv_library"}, got
        return
    want = N.route_table(2, *run.hw, ws=run.ws)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    print(f"\n{run.case}: library-routed layers {sorted(k for k, v in got.items() if v in ('library', 'conv_library'))}")
    if run.case == "routes-bf16":
        assert set(want.values()) <= set(N.LINEAR_ROUTES + N.MLP_ROUTES + N.CONV_ROUTES)
        assert N.route_table(2, 64, 96) != want, "the toy grid has the benchmark's routes: the routes case adds nothing"
        grid, bench = N.smallest_grid_with_routes_of(*BENCH)
        assert grid == run.hw and got == bench
        assert grid[0] * grid[1] < BENCH[1] * BENCH[2]
        assert {"row_gemm", "tiled_gemm", "row_mlp", "tiled_mlp", "conv_mfma", "conv_igemm"} <= set(bench.values())
        print(f"\nroutes case: grid {grid}; table {bench}")


# ------------------------------------------------------------------------------------------------ float64
def test_nodes_against_float64(run):
    bf = run.bf16
    T = Tally(run.case)
    bar = T.bar

    def near(got, ref, what, grad=False):
        """an activation-typed map: the bf16-map bars, or the fp32 flavour's output / gradient bar"""
        if bf:
            got, ref = got.detach().double(), ref.detach().double()
            assert got.shape == ref.shape, (what, got.shape, ref.shape)
            bar(float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)), 6e-3, f"{what} (max)", "bf16 map, max")
            bar(rel(got, ref), 3e-3, f"{what} (2-norm)", "bf16 map, 2-norm")
        else:
            assert got.shape == ref.shape, (what, got.shape, ref.shape)
            bar(rel(got, ref), 1e-4 if grad else 1e-5, what, "fp32 grad" if grad else "fp32 out")

    def wgrad(got, ref, what, route, limit=5e-4, key="GEMM / conv dW, db"):
        if not bf:
            bar(rel(got, ref), 1e-4, what, "fp32 grad")
        elif route in ("library", "conv_library"):
            near(got, ref, what + " (library: rounded to bf16)")
        else:
            bar(rel(got, ref), limit, what, key)

    def composed(v, key, what, lower=False):
        if bf:
            bar(v, COMPOSED_BARS[key], what, key, lower)
        elif not lower:
            bar(v, 1e-5 if key.endswith((" y", " y-x", " y-res")) else 1e-4, what, "fp32 composed " + ("out" if key.endswith((" y", " y-x", " y-res")) else "grad"))

    for node in run.rec.nodes:
        r = replay(run, node)
        a, o, k, g = node.args, node.opts, node.kind, r.grads
        what = f"{k} {node.name}"
        if k == "ln":
            x = a["x"]
            mask = None if o["real"] is None else (x.shape[1], x.shape[2], o["real"][0], o["real"][1])
            if o.get("unit"):
                y64, (dx64,) = N.node(lambda x: N.ln(x, None, None, o["eps"]), (x,), node.dy)
            else:
                y64, (dx64, dg64, db64) = N.node(lambda x, g_, b_: N.ln(x, g_, b_, o["eps"], mask), (x, a["g"], a["b"]), node.dy)
                for s, ref in (("g", dg64), ("b", db64)):
                    bar(rel(g[s], ref), 2e-3 if bf else 1e-4, f"{what} d{s}", "LayerNorm dgamma, dbeta" if bf else "fp32 grad")
            near(r.y, y64, f"{what} y")
            near(g["x"], dx64, f"{what} dx", grad=True)
            if mask is not None:
                pad = N.row_mask(x.shape[0], *mask, x.device).view(x.shape[0], x.shape[1], x.shape[2], 1) == 0
                assert not (r.y * pad).any() and not (g["x"] * pad).any(), f"{what}: padding rows are not zero"
        elif k == "attn":
            y64, (dq64, db64) = N.node(lambda q, b_: N.attn_core(q, b_, o["heads"], o["ws"], o["shift"]), (a["qkv"], a["bias"]), node.dy)
            bar(rel(r.y, y64), 6e-3 if bf else 2e-6, f"{what} out", "attention out")
            bar(rel(g["qkv"], dq64), 1.5e-2 if bf else 5e-6, f"{what} dqkv", "attention dqkv, dbias")
            bar(rel(g["bias"], db64), 1.5e-2 if bf else 5e-6, f"{what} dbias", "attention dqkv, dbias")
            C = a["qkv"].shape[-1] // 3
            for i, s in enumerate("qkv"):
                bar(rel(g["qkv"][..., i * C:(i + 1) * C], dq64[..., i * C:(i + 1) * C]), 2e-2 if bf else 5e-6, f"{what} d{s}", "attention dq / dk / dv")
        elif k == "table":
            same(r.y, a["table"][a["index"]], f"{what} rows")
            bar(rel(g["table"], N.table_rows_grad(a["index"], a["table"].shape[0], node.dy.double())), 1e-5, f"{what} dtable", "table gradient")
        elif k == "linear":
            w64, has_b, has_r = N.gemm_w(a["w"], bf), a["b"] is not None, a["res"] is not None
            y64, gr = N.node(N.linear, (a["x"], w64, a["b"], a["res"]), node.dy)
            near(r.y, y64, f"{what} y [{node.route}]")
            near(g["x"], gr[0], f"{what} dx [{node.route}]", grad=True)
            wgrad(g["w"], gr[1], f"{what} dW [{node.route}]", node.route)
            if has_b:
                wgrad(g["b"], gr[2], f"{what} db [{node.route}]", node.route)
            if has_r:
                same(g["res"], node.dy, f"{what} dres")
        elif k == "mlp":
            w1, w2 = N.gemm_w(a["w1"], bf), N.gemm_w(a["w2"], bf)
            y64, gr = N.node(lambda x, w1_, b1, w2_, b2, res: N.mlp(x, w1_, b1, w2_, b2, res, round_hidden=bf),
                             (a["x"], w1, a["b1"], w2, a["b2"], a["res"]), node.dy)
            res = a["res"].double()
            composed(rel(r.y.double() - res, y64 - res), "mlp y-res", f"{what} y - res [{node.route}]")
            bar(rel(y64 - res, res), 0.05, f"{what}: own part against the residual", "own part >= 5 %", lower=True)
            composed(rel(g["x"], gr[0]), "mlp dx", f"{what} dx [{node.route}]")
            for s, ref in (("w1", gr[1]), ("w2", gr[3])):
                composed(rel(g[s], ref), "mlp dW", f"{what} d{s} [{node.route}]")
            for s, ref in (("b1", gr[2]), ("b2", gr[4])):
                composed(rel(g[s], ref), "mlp db", f"{what} d{s} [{node.route}]")
            same(g["res"], node.dy, f"{what} dres")
        elif k == "conv":
            y64, dx64, dw64, _ = N.UN.conv_node(a["x"], a["w"], None, dy=node.dy, round_weight=bf)
            near(r.y, y64, f"{what} y [{node.route}]")
            near(g["x"], dx64, f"{what} dx [{node.route}]", grad=True)
            wgrad(g["w"], dw64, f"{what} dw [{node.route}]", node.route)
        elif k == "inorm":
            fn = lambda sign: (lambda x, g_, b_, res: N.inorm_act(x, g_, b_, o["eps"], o["slope"], res, sign_of=sign))  # noqa: E731
            ops = (a["x"], a["g"], a["b"], a["res"])
            own, _ = N.node(fn(None), ops, node.dy)            # forward: the reference's own decisions (an output wrongly scaled shows)
            _, gr = N.node(fn(r.y), ops, node.dy)              # backward: the LeakyReLU sign of the stored output
            lim, key = (1.5e-2, "instance norm") if bf else (None, None)
            for got, ref, s, grad in ((r.y, own, "y", False), (g["x"], gr[0], "dx", True), (g["g"], gr[1], "dgamma", True),
                                      (g["b"], gr[2], "dbeta", True), (g["res"], gr[3], "dres", True)):
                if ref is not None:
                    bar(rel(got, ref), lim if bf else (1e-4 if grad else 1e-5), f"{what} {s}", key if bf else ("fp32 grad" if grad else "fp32 out"))
        else:
            mod, x = node.module, a["x"]
            names = N.BLOCK_PARAMS if k == "block" else N.MERGE_PARAMS
            P = N.module_leaves(mod, names, rounded=bf)
            x64 = x.double().requires_grad_(True)
            with torch.enable_grad():
                if k == "block":
                    yr = N.block(x64, P, mod.heads, mod.ws, mod.shift, mod.norm1.eps, real=o["real"], round_hidden=bf)
                else:
                    yr = N.merge(x64, P, mod.norm.eps)
                gr = torch.autograd.grad(yr, [x64] + [P[n] for n in names], node.dy.double())
            yr = yr.detach()
            composed(rel(r.y, yr), f"{k} y", f"{what} y")
            composed(rel(g["x"], gr[0]), f"{k} dx", f"{what} dx")
            if k == "block":
                x0, d0 = x.double(), node.dy.double()
                bar(rel(yr - x0, x0), 0.05, f"{what}: own part against x", "own part >= 5 %", lower=True)
                composed(rel(r.y.double() - x0, yr - x0), "block y-x", f"{what} y - x")
                composed(rel(g["x"].double() - d0, gr[0] - d0), "block dx-dy", f"{what} dx - dy")
            for n, ref in zip(names, gr[1:]):
                assert g[n] is not None, f"{what}: {n} got no gradient"
                if k == "block" and n == "qkv.weight":       # (through dS = P (dP - D): on its own key; it meets 3e-2 here, no cosine bar needed)
                    composed(rel(g[n], ref), "block dqkv.weight", f"{what} d{n}")
                else:
                    composed(rel(g[n], ref), f"{k} dparam", f"{what} d{n}")
    T.done()


# ------------------------------------------------------------------------------------------------ wiring
def to_param(name, module, slot, g):
    """a leaf node's replayed gradient of the operand it was given, in the parameter's own layout"""
    if slot == "w" and name == "patch_embed":
        fs, C = module.weight.shape[0], module.weight.shape[1]
        return g.view(fs, 2, 2, -1)[..., :C].permute(0, 3, 1, 2)
    if slot == "w" and name.endswith("transp_conv"):
        cin, cout = module.weight.shape[0], module.weight.shape[1]
        return g.view(2, 2, cout, cin).permute(3, 2, 0, 1)
    if slot == "w" and name == "out":
        return g.view(module.weight.shape)
    return g


def node_params(run, node):
    """{slot: (parameter name, parameter, module)} of a leaf node"""
    m, k = run.model, node.kind
    if k == "table":
        return {"table": (node.name, m.get_parameter(node.name), None)}
    if k == "mlp":
        pre = node.name[:-len("mlp")]
        return {s: (pre + n, m.get_parameter(pre + n), None) for s, n in (("w1", "fc1.weight"), ("b1", "fc1.bias"), ("w2", "fc2.weight"), ("b2", "fc2.bias"))}
    if k in ("attn", "block", "merge") or node.opts.get("unit"):
        return {}
    mod = m.get_submodule(node.name)
    slots = {"ln": (("g", "weight"), ("b", "bias")), "inorm": (("g", "weight"), ("b", "bias")), "conv": (("w", "weight"),),
             "linear": (("w", "weight"), ("b", "bias"))}[k]
    return {s: (f"{node.name}.{n}", getattr(mod, n), mod) for s, n in slots if getattr(mod, n, None) is not None}


LIB = "library"      # stands for a producer that is no recorded node (the fp32 flavour's bare matmuls / library LayerNorm)


def edge(run, got, want, what, *producers):
    """`got`, the gradient a node's output received in the network, is `want`, what the replays of its consumers produced: bit for bit;
    if one of the producers runs on a library route (no fixed-order promise) to a bf16 / fp32 rounding instead"""
    assert got is not None and want is not None, f"{what}: missing"
    want = want.reshape(got.shape)
    if any(p is LIB or from_library(run, p) for p in producers):
        lim = 1e-2 if run.bf16 else 1e-5
        assert got.dtype == want.dtype and rel(got, want) <= lim, f"{what}: {rel(got, want):.2e} > {lim:.0e} (library route)"
    else:
        same(got, want, what)


def res_block_edges(run, pre, dy_out, producers):
    """the edges inside a ResBlock whose output received dy_out from `producers`: (the gradient of its input, its producers)"""
    rec = run.rec
    G = lambda n: replay(run, n).grads  # noqa: E731
    c1, n1, c2, n2 = (rec[pre + s] for s in ("conv1", "norm1", "conv2", "norm2"))
    edge(run, n2.dy, dy_out, f"{pre}norm2: the block's dy", *producers)
    edge(run, c2.dy, G(n2)["x"], f"{pre}: norm2 dx -> conv2", n2)
    edge(run, n1.dy, G(c2)["x"], f"{pre}: conv2 dx -> norm1", c2)
    edge(run, c1.dy, G(n1)["x"], f"{pre}: norm1 dx -> conv1", n1)
    if any(n.name == pre + "conv3" for n in rec.nodes):
        c3, n3 = rec[pre + "conv3"], rec[pre + "norm3"]
        edge(run, n3.dy, G(n2)["res"], f"{pre}: norm2 dres -> norm3 (the skip junction)", n2)
        edge(run, c3.dy, G(n3)["x"], f"{pre}: norm3 dx -> conv3", n3)
        return (G(c1)["x"], G(c3)["x"]), (c1, c3)
    return (G(c1)["x"], G(n2)["res"]), (c1, n2)


def up_block_edges(run, pre, dy_out, producers):
    """the edges inside an UpBlock: (gradient of its input x, producers, gradient of its skip, producers)"""
    rec = run.rec
    (da, db), prods = res_block_edges(run, pre + "conv_block.", dy_out, producers)
    dcat = da + db                                              # (two consumers of cat([up, skip]): conv1 and conv3)
    B, H2, W2, C2 = dcat.shape
    cout = C2 // 2
    dup = dcat[..., :cout].reshape(B, H2 // 2, 2, W2 // 2, 2, cout).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4 * cout)
    dskip = dcat[..., cout:]
    if run.bf16:
        t = rec[pre + "transp_conv"]
        edge(run, t.dy, dup, f"{pre}: cat[..., :cout] -> transposed-convolution GEMM", *prods)
        return replay(run, t).grads["x"].reshape(B, H2 // 2, W2 // 2, -1), (t,), dskip, prods
    wt = run.model.get_submodule(pre + "transp_conv").weight    # fp32 flavour: a bare library matmul, no node
    return (dup @ wt.detach().permute(0, 2, 3, 1).reshape(wt.shape[0], 4 * cout).t()).reshape(B, H2 // 2, W2 // 2, -1), (LIB,), dskip, prods


def test_wiring_is_bit_identical(run):
    rec, m = run.rec, run.model
    G = lambda name: replay(run, rec[name]).grads  # noqa: E731
    for blk in rec.of("block"):
        b = blk.name
        n1, qkv, tab, att, proj, n2, mlp = (rec[f"{b}.{s}"] for s in ("norm1", "qkv", "relative_position_bias_table", "attn", "proj", "norm2", "mlp"))
        heads, Nt = att.opts["heads"], att.opts["ws"] ** 2
        edge(run, qkv.dy, G(att.name)["qkv"], f"{b}: attention dqkv -> qkv Linear", att)
        edge(run, tab.dy, G(att.name)["bias"].permute(1, 2, 0).reshape(Nt * Nt, heads), f"{b}: attention dbias -> table rows", att)
        edge(run, n1.dy, G(qkv.name)["x"], f"{b}: qkv dx -> norm1", qkv)          # (no per-block padding in any case here: same grid)
        edge(run, att.dy, G(proj.name)["x"], f"{b}: proj dx -> attention", proj)
        edge(run, n2.dy, G(mlp.name)["x"], f"{b}: MLP dx -> norm2", mlp)
        same(mlp.dy, blk.dy, f"{b}: the block's dy -> MLP")
        assert proj.args["res"] is not None, f"{b}: the residual is not in the projection's epilogue"
        edge(run, proj.dy, G(n2.name)["x"] + G(mlp.name)["res"], f"{b}: norm2 dx + MLP dres -> proj", n2, mlp)
        edge(run, G(b)["x"], G(n1.name)["x"] + G(proj.name)["res"], f"{b}: norm1 dx + proj dres = the block's dx", blk, n1, proj)
    for i in range(4):
        b0, b1, mg = rec[f"stages.{i}.0"], rec[f"stages.{i}.1"], rec[f"merges.{i}"]
        edge(run, b0.dy, G(b1.name)["x"], f"stage {i}: block 1 dx -> block 0", b1)
        h, w = mg.args["x"].shape[1], mg.args["x"].shape[2]
        edge(run, b1.dy[:, :h, :w].contiguous(), G(mg.name)["x"], f"stage {i}: merging dx -> block 1 (the crop)", mg)
        crop = torch.zeros_like(b1.dy[..., :1])
        crop[:, :h, :w] = 1
        assert not (b1.dy * (1 - crop)).any(), f"stage {i}: the padding tokens of the stage's output took a gradient"
        red, lnm = rec[f"merges.{i}.reduction"], rec[f"merges.{i}.norm"]
        same(red.dy, mg.dy, f"merges.{i}: dy -> reduction")
        edge(run, lnm.dy, G(red.name)["x"], f"merges.{i}: reduction dx -> norm", red)
    head = rec["out"]
    same(head.dy, run.dy.to(head.dy.dtype), "out: the network's dy")
    # the decoder, from the head down: every convolution, instance norm and transposed-convolution GEMM; at a cat([up, skip]) the
    # channel slices; where a tensor has two consumers the sum of what both produced (two terms: the order cannot matter)
    d, prods, skips = G("out")["x"], (head,), {}
    for dec in ("decoder1", "decoder2", "decoder3", "decoder4", "decoder5"):
        d, prods, dskip, sprods = up_block_edges(run, dec + ".", d, prods)
        skips[dec] = (dskip, sprods)
    dh = {}                                                     # hidden state -> ((gradient terms), producers)
    dh[4] = res_block_edges(run, "encoder10.", d, prods)
    dh[3] = ((skips["decoder5"][0],), skips["decoder5"][1])
    for k, (enc, dec) in enumerate((("encoder2", "decoder2"), ("encoder3", "decoder3"), ("encoder4", "decoder4"))):
        dh[k] = res_block_edges(run, enc + ".", *skips[dec])
    (xa, xb), xprods = res_block_edges(run, "encoder1.", *skips["decoder1"])
    # the hidden states: the token stream's tensor (patch embedding / merging k - 1) feeds hidden.k and the first block of stage k
    for k in range(5):
        src = rec["patch_embed"] if k == 0 else rec[f"merges.{k - 1}"]
        terms, hp = dh[k]
        dhk = terms[0] if len(terms) == 1 else terms[0] + terms[1]
        if any(n.name == f"hidden.{k}" for n in rec.nodes):
            hid = rec[f"hidden.{k}"]
            edge(run, hid.dy, dhk, f"hidden.{k}: the decoder's gradient", *hp)
            dsrc, sp = G(hid.name)["x"].reshape(src.out.shape), [hid]
        else:                                                    # fp32 flavour, 384 features: the library's LayerNorm, no node
            assert not run.bf16 and k == 4
            t = src.out.detach().clone().requires_grad_(True)
            torch.nn.functional.layer_norm(t, t.shape[-1:]).backward(dhk.reshape(t.shape))
            dsrc, sp = t.grad, [LIB]
        if k < 4:
            b0 = rec[f"stages.{k}.0"]
            dsrc = dsrc + G(b0.name)["x"][:, :src.out.shape[1], :src.out.shape[2]]
            sp.append(b0)
        edge(run, src.dy, dsrc, f"{src.name}: hidden.{k} dx" + (f" + stages.{k}.0 dx (cropped)" if k < 4 else ""), *sp)
    # the input: encoder1's two convolutions and the patch embedding (through the even-channel padding and the 2 x 2 patch view) --
    # three terms, summed in the activation type in an order autograd chooses: one of the three pairings
    pe = rec["patch_embed"]
    B, H, W, C = run.x.shape
    xc = G("patch_embed")["x"].reshape(B, H // 2, W // 2, 2, 2, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, -1)[..., :C]
    sums = [((p + q) + r).to(run.dx.dtype) for p, q, r in ((xa, xb, xc), (xa, xc, xb), (xb, xc, xa))]
    if any(from_library(run, n) for n in (pe,) + tuple(xprods)):
        assert min(rel(run.dx, t) for t in sums) <= (1e-2 if run.bf16 else 1e-5), "the network's dx"
    else:
        assert any(torch.equal(run.dx, t) for t in sums), f"the network's dx is no ordering of its three terms ({min(rel(run.dx, t) for t in sums):.2e})"
    # the network's p.grad is the leaf nodes' replayed parameter gradient; every parameter belongs to exactly one leaf node
    owner = {}
    for node in rec.nodes:
        for slot, (pname, p, mod) in node_params(run, node).items():
            assert pname not in owner, f"{node.name} {slot}: {pname} already taken by {owner[pname]}"
            owner[pname] = node.name
            got = to_param(node.name, mod, slot, replay(run, node).grads[slot]).to(p.dtype)
            if from_library(run, node):
                assert rel(got, run.g_none[pname]) <= 1e-2, f"{pname}: {rel(got, run.g_none[pname]):.2e}"
            else:
                same(got.contiguous(), run.g_none[pname].contiguous(), f"{node.name} {slot}: p.grad of {pname}")
    names = [n for n, _ in m.named_parameters()]
    missing = [n for n in names if n not in owner]
    assert len(names) == 203 and len(rec.nodes) == (140 if run.bf16 else 134)
    if run.bf16:
        assert not missing and len(owner) == 203, missing
    else:
        assert sorted(missing) == sorted(f"decoder{i}.transp_conv.weight" for i in range(1, 6)) and len(owner) == 198, missing
    # composed nodes: their parameter gradients are the leaf nodes'
    for comp in rec.of("block", "merge"):
        if from_library(run, comp):
            continue
        for n, gc in replay(run, comp).grads.items():
            if n != "x":
                same(gc, run.g_none[f"{comp.name}.{n}"], f"{comp.name}: {n} of the composed replay")


# ------------------------------------------------------------------------------------------------ sink route
def test_sink_route_adds_into_grad(run):
    from py4cast_amd.trainer import FlatDDP

    if run.case != "toy-ws7-bf16":
        return
    m = run.model
    g = torch.Generator(device=run.x.device).manual_seed(11)
    prefill = {n: (torch.rand(p.shape, device=p.device, generator=g) + 0.5) * (1 - 2 * (torch.rand(p.shape, device=p.device, generator=g) < 0.5))
               for n, p in m.named_parameters()}
    for n, p in m.named_parameters():
        p.grad = prefill[n].clone()
    step(m, run.x, run.dy)
    for n, p in m.named_parameters():
        same(p.grad, prefill[n] + run.g_none[n], f"prefilled .grad: {n}")
    ddp = FlatDDP(m, 1)
    for n, p in m.named_parameters():
        assert p.grad.data_ptr() >= ddp.flat_grad.data_ptr(), n
        p.grad.copy_(prefill[n])
    step(m, run.x, run.dy)
    for n, p in m.named_parameters():
        same(p.grad, prefill[n] + run.g_none[n], f"FlatDDP .grad: {n}")
    m.zero_grad(set_to_none=True)
