"""
UNETR++ (py4cast_amd/unetrpp.py) transformer-block nodes inside the network: one forward / backward of UNetRPPMI355X (bf16) with these
entry points of every transformer block recorded -- ``ops_rows.add_layer_norm`` (aln: x + pos_embed and its LayerNorm), ``ops_ts.epa_core``
(epa), ``ops_ts.merge_published`` (merge, published block only), ``ops_gemm.cat_linear_res`` (catlin: t + gamma * [out_proj(x_sa),
out_proj2(x_ca)]) and ``ops_gemm.batch_norm_act`` (bn: conv51's two batch norms with LeakyReLU 0.01; norm2 with the skip as residual,
its passthrough to conv8 and the channel-dropout table) -- and the ``backward`` of their autograd Functions.  The calls are untouched.
Not recorded yet: the convolutions and linears (qkvv, conv51, conv8, the stem and down-samplings), the group / instance norms, the
full-resolution blocks and the up-sampling.  Then per node:

* replay: the node alone on its recorded inputs and incoming gradients, with fresh parameter leaves, gives the in-network outputs and
  gradients BIT FOR BIT;
* float64: the replay against tests/unetrpp_nodes.py's references (which tests/test_unetrpp_nodes_cpu.py composes into the oracle's
  EPA block): bf16 maps <= 6e-3 of the largest magnitude per element and <= 3e-3 in the 2-norm (the four slices of dqkvv each against
  its own magnitude), weight / bias / positional-table gradients <= 5e-4, LayerNorm / batch-norm gamma / beta, temperatures and the
  layer scale gamma <= 5e-3, running mean / var <= 1e-4 with num_batches_tracked advanced by one; the merge is an exact permutation both
  ways.  bn: the forward against float64's own LeakyReLU decisions and the recorded dropout draw applied per (sample, channel); the
  residual's gradient against dz + the gradient the passthrough output received from conv8 (a lost addition shows);
* wiring: x_sa -> merge (or the restated view) -> catlin's first operand, x_ca -> catlin's second, aln's t -> catlin's residual: the
  gradient each producer received is, bit for bit, what its consumer returned; conv51.norm2 takes a residual, hands it on and received
  a passthrough gradient; its dropout table is a 0 / 1 draw per (sample, channel) with factor 1 / (1 - p) exactly when the published
  block trains with p > 0, and absent otherwise;
* ownership: every parameter of these nodes belongs to exactly one node and the network's p.grad is that node's replay gradient; in a
  block whose attention runs on the node every parameter but those of the unrecorded convolutions is owned; E = F: F is E, the state
  dict's F.* keys are E's tensors, and the parameter is counted once;
* sink route: the same backward with every .grad of the model pre-filled, and under FlatDDP as bench.py builds it: p.grad = prefill +
  the first run's gradient, bit for bit, for every parameter (E.weight's gradient is added in place by epa_core itself).  The channel
  dropout in front of conv8 draws from the default generator: every run is seeded alike, so all runs see the same draw.

Cases: a toy published block with conv8 dropout 0.1 in training mode (the fourth stage, 4 tokens with p = 4, takes the composed EPA,
not the node: the schedule says so), the same with the restated block, and the benchmark size with bench.model_settings("UNetRPP",
"bf16"): 2 x 512 x 512, 69 input channels handed as the 96-channel bf16 rows of the rollout's build_x, 60 outputs, hidden size 1024.

Measured at the benchmark size (worst node / bar; the float64 test prints them): aln / catlin bf16 maps 5.8e-3 / 6e-3 per element and
2.4e-3 / 3e-3 in the 2-norm (the bf16 rounding of the stored maps), positional-table gradient 3.9e-6 / 5e-4, LayerNorm gamma / beta
1.7e-7 / 5e-3, out_proj / out_proj2 weight and bias 2.1e-7 / 5e-4, layer scale 2.0e-7 / 5e-3, batch-norm gamma / beta 2.1e-7 / 5e-3,
running statistics 4.6e-8 / 1e-4 (bn maps within the bf16 map values above); epa x_sa 3.5e-3 / 6e-3 and 1.7e-3 / 3e-3,
x_ca 3.8e-3 / 6e-3 and 1.7e-3 / 3e-3, dv_ca and dv_sa <= 4.2e-3 / 6e-3 and 2.4e-3 / 3e-3, dq 7.0e-3 / 1.2e-2 and 2.9e-3 / 5e-3, dk 8.0e-3
/ 1.2e-2 and 3.0e-3 / 5e-3 (the wider bars of tests/unetrpp_nodes.py::EPA_BARS: set from these runs, the toy cases reach 3.2e-3 in the
2-norm), E.weight 2.3e-4 / 5e-4, E.bias 2.6e-4 / 5e-4, temperature 7.2e-7 / 5e-3, temperature2 3.4e-5 / 5e-3.  The whole file takes
about 8 s on one MI355X.
"""
import copy
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import unetrpp_nodes as UN  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {
    # name: (B, H, W, in_channels, out_channels, settings)
    "toy-published": (2, 64, 64, 16, 8, dict(hidden_size=256, num_heads_encoder=4, num_heads_decoder=4, depths=(2, 1, 1, 1),
                                             encoder_proj_sizes=(16, 16, 8, 4), decoder_proj_size=16, linear_upsampling=True,
                                             activation_dtype="bf16", published_block=True, conv8_dropout=0.1)),
    "toy-restated": (2, 64, 64, 16, 8, dict(hidden_size=256, num_heads_encoder=4, num_heads_decoder=4, depths=(2, 1, 1, 1),
                                            encoder_proj_sizes=(16, 16, 8, 4), decoder_proj_size=16, linear_upsampling=True,
                                            activation_dtype="bf16", published_block=False, conv8_dropout=0.0)),
    "bench": (2, 512, 512, 69, 60, None),
}

GRAD_SLOTS = {"aln": {"x": 0, "add": 1, "gamma": 2, "beta": 3},
              "epa": {"qkvv": 0, "W": 1, "bias": 2, "t1": 3, "t2": 4},
              "merge": {"x_sa": 0},
              "catlin": {"xa": 0, "wa": 1, "ba": 2, "xb": 3, "wb": 4, "bb": 5, "res": 6, "gamma": 7},
              "bn": {"y": 0, "gamma": 2, "beta": 3, "res": 4}}


def blocks(model):
    """the transformer blocks in the order UNetRPPMI355X.forward runs them: the four encoder stages, then decoder5 / 4 / 3"""
    out = [b for st in model.stages for b in st]
    for up in (model.decoder5, model.decoder4, model.decoder3):
        out += list(up.decoder_block[0])
    return out


def schedule(model, B, dev):
    """[(kind, block, module)] the bf16 forward calls, derived from the routing predicates of unetrpp.py on probe tensors of each block's
    shapes (module: the batch norm of a "bn" call, else None)"""
    from py4cast_amd import ops_gemm as G
    from py4cast_amd import ops_rows as R
    from py4cast_amd import ops_ts as TS

    s = []
    for blk in blocks(model):
        epa = blk.epa_block
        N, C = blk.pos_embed.shape[1:]
        h, d = epa.heads, C // epa.heads
        rows = torch.empty(B, N, C, dtype=torch.bfloat16, device=dev)
        assert R.add_layer_norm_supported(rows) and C % 16 == 0, "every block of these cases runs features-last"
        s.append(("aln", blk, None))
        if TS.epa_core_ok(torch.empty(B, N, 4, h, d, dtype=torch.bfloat16, device=dev), epa.E.out_features):
            s.append(("epa", blk, None))
        if epa.published and TS.merge_published_ok(rows.view(B, N, h, d).permute(0, 2, 1, 3)):
            s.append(("merge", blk, None))
        if G.supported(rows, epa.out_proj.weight) and epa.out_proj.weight.shape[0] % 8 == 0:
            s.append(("catlin", blk, None))
        side = int(round(N ** 0.5))      # (square grids in these cases)
        r51 = blk.conv51
        if (isinstance(r51.norm1, torch.nn.BatchNorm2d) and not r51.down and C % 8 == 0 and C <= 1024
                and G.conv_supported(rows.view(B, side, side, C), r51.conv1.weight)):
            s += [("bn", blk, r51.norm1), ("bn", blk, r51.norm2)]      # (ResBlock._forward: the implicit-GEMM route)
    return s


COUNTS = {  # per case: calls of each kind (the toy's fourth stage has 4 tokens and p = 4: no epa / merge node there)
    "toy-published": {"aln": 14, "epa": 13, "merge": 13, "catlin": 14, "bn": 28},
    "toy-restated": {"aln": 14, "epa": 13, "merge": 0, "catlin": 14, "bn": 28},
    "bench": {"aln": 21, "epa": 21, "merge": 21, "catlin": 21, "bn": 42},
}


def _clone(t):
    return None if t is None else t.detach().clone()


class Node:
    def __init__(self, kind, blk, args, module=None):
        self.kind, self.blk, self.args, self.module = kind, blk, args, module
        self.out = self.gout = self.gin = None
        self.pre = copy.deepcopy(module) if module is not None else None      # the batch norm before the call (running statistics)
        self.post = None

    def grad(self, slot):
        return self.gin[GRAD_SLOTS[self.kind][slot]]

    def params(self):
        """{slot: leaf parameter} of this node"""
        b, e = self.blk, self.blk.epa_block
        return {"aln": {"add": b.pos_embed, "gamma": b.norm.weight, "beta": b.norm.bias},
                "epa": {"W": e.E.weight, "bias": e.E.bias, "t1": e.temperature, "t2": e.temperature2},
                "merge": {},
                "catlin": {"wa": e.out_proj.weight, "ba": e.out_proj.bias, "wb": e.out_proj2.weight, "bb": e.out_proj2.bias,
                           "gamma": b.gamma},
                "bn": {} if self.module is None else {"gamma": self.module.weight, "beta": self.module.bias}}[self.kind]


class Recorder:
    """``with Recorder(model, expected) as rec: ...`` -- rec.nodes in call order; each call checked against the schedule"""

    def __init__(self, expected):
        self.expected, self.nodes, self._ctx, self._keep = expected, [], {}, []

    def _begin(self, kind, owner, args):
        i = len(self.nodes)
        assert i < len(self.expected), f"node {i} ({kind}): more calls than the schedule has"
        ekind, blk, mod = self.expected[i]
        assert kind == ekind, f"node {i}: expected {ekind}, got {kind}"
        if kind == "bn":
            assert owner is mod, f"node {i} (bn): not the scheduled batch norm"
        elif owner is not None:
            assert owner is blk.pos_embed or owner is blk.epa_block.E.weight or owner is blk.epa_block.out_proj.weight, \
                f"node {i} ({kind}): not the scheduled block's"
        return Node(kind, blk, {k: _clone(v) for k, v in args.items()}, mod)

    def _end(self, node, outs):
        node.out = [_clone(o) for o in outs]
        if node.module is not None:
            node.post = copy.deepcopy(node.module)
        self.nodes.append(node)
        self._ctx[id(outs[0].grad_fn)] = node
        self._keep.append(outs[0].grad_fn)

    def _wrap_backward(self, fn_cls):
        orig = fn_cls.__dict__["backward"].__func__
        rec = self

        def backward(ctx, *grads):
            node = rec._ctx.get(id(ctx))
            if node is not None:
                node.gout = [_clone(g) for g in grads]
            res = orig(ctx, *grads)
            res = res if isinstance(res, tuple) else (res,)
            if node is not None:
                node.gin = [_clone(r) if isinstance(r, torch.Tensor) else None for r in res]
            return res if len(res) > 1 else res[0]

        self._mp.setattr(fn_cls, "backward", staticmethod(backward))

    def __enter__(self):
        from py4cast_amd import ops_gemm as G
        from py4cast_amd import ops_rows as R
        from py4cast_amd import ops_ts as TS

        rec = self
        aln0, epa0, merge0, cat0 = R.add_layer_norm, TS.epa_core, TS.merge_published, G.cat_linear_res

        def add_layer_norm(x, add, gamma, beta, eps=1e-5):
            node = rec._begin("aln", add, {"x": x, "add": add, "gamma": gamma, "beta": beta})
            node.eps = eps
            out = aln0(x, add, gamma, beta, eps)
            rec._end(node, out)
            return out

        def epa_core(qkvv, W, bias, t1, t2):
            node = rec._begin("epa", W, {"qkvv": qkvv, "W": W, "bias": bias, "t1": t1, "t2": t2})
            out = epa0(qkvv, W, bias, t1, t2)
            rec._end(node, out)
            return out

        def merge_published(x_sa):
            node = rec._begin("merge", None, {"x_sa": x_sa})
            out = merge0(x_sa)
            rec._end(node, [out])
            return out

        def cat_linear_res(xa, wa, ba, xb, wb, bb, res, gamma=None):
            assert gamma is not None, "the block's layer scale rides in the node"
            node = rec._begin("catlin", wa, dict(xa=xa, wa=wa, ba=ba, xb=xb, wb=wb, bb=bb, res=res, gamma=gamma))
            out = cat0(xa, wa, ba, xb, wb, bb, res, gamma=gamma)
            rec._end(node, [out])
            return out

        bn0 = G.batch_norm_act

        def batch_norm_act(y, stats, bn, slope=1.0, res=None, res_passthrough=False, mul=None, mul_factor=1.0):
            node = rec._begin("bn", bn, {"y": y, "stats": stats, "res": res, "mul": mul})
            node.opts = dict(slope=float(slope), res_passthrough=bool(res_passthrough), mul_factor=float(mul_factor))
            out = bn0(y, stats, bn, slope, res, res_passthrough, mul, mul_factor)
            rec._end(node, list(out) if res_passthrough else [out])
            return out

        self._mp = pytest.MonkeyPatch()
        self._mp.setattr(R, "add_layer_norm", add_layer_norm)
        self._mp.setattr(TS, "epa_core", epa_core)
        self._mp.setattr(TS, "merge_published", merge_published)
        self._mp.setattr(G, "cat_linear_res", cat_linear_res)
        self._mp.setattr(G, "batch_norm_act", batch_norm_act)
        for fn_cls in (R._AddLayerNorm, TS._EpaCore, TS._MergePublished, G._CatLinearRes, G._BatchNormAct):
            self._wrap_backward(fn_cls)
        return self

    def __exit__(self, exc_type, exc, tb):
        self._mp.undo()
        self._keep = []
        if exc_type is None:
            assert len(self.nodes) == len(self.expected), f"{len(self.nodes)} node calls, the schedule has {len(self.expected)}"
        return False


def make_model(case, dev):
    from py4cast_amd.unetrpp import UNetRPPMI355X, UNetRPPSettings

    B, H, W, cin, cout, s = CASES[case]
    if s is None:
        import bench

        s = bench.model_settings("UNetRPP", "bf16")
    torch.manual_seed(0)
    m = UNetRPPMI355X(cin, cout, (H, W), UNetRPPSettings(**s)).to(dev).train()
    with torch.no_grad():     # (the published initialisation -- gamma 1e-6, zero table, unit temperatures, E's small bias -- hides too much)
        for n, p in m.named_parameters():
            if n.endswith("gamma"):
                p.uniform_(0.3, 0.7)
            elif n.endswith("pos_embed"):
                p.normal_(0, 0.1)
            elif "temperature" in n:
                p.uniform_(0.5, 3.0)
            elif n.endswith("E.bias"):
                p.uniform_(-0.5, 0.5)
    g = torch.Generator(device=dev).manual_seed(7)
    fmt = m.rollout_input_format
    if case == "bench":        # the rows build_x emits: bf16, zero-padded to the 32-channel multiple
        x = torch.zeros(B, H, W, fmt[1], dtype=torch.bfloat16, device=dev)
        x[..., :cin] = torch.randn(B, H, W, cin, device=dev, generator=g)
    else:
        x = torch.randn(B, H, W, cin, device=dev, generator=g).to(torch.bfloat16)
    dy = torch.randn(B, H, W, cout, device=dev, generator=g).to(torch.bfloat16)
    return m, x, dy


def step(m, x, dy):
    torch.manual_seed(1234)       # the conv8 dropout's draw: the same in every run
    y = m(x)
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach()


@pytest.fixture(scope="module", params=list(CASES))
def run(request, gpu_device):
    torch.cuda.empty_cache()
    m, x, dy = make_model(request.param, gpu_device)
    expected = schedule(m, x.shape[0], gpu_device)
    got = {k: sum(e[0] == k for e in expected) for k in COUNTS[request.param]}
    assert got == COUNTS[request.param], got
    with Recorder(expected) as rec:
        y = step(m, x, dy)
    for n in rec.nodes:
        assert n.gout is not None and n.gin is not None, f"{n.kind}: no backward recorded"
    g_none = {name: p.grad.detach().clone() for name, p in m.named_parameters()}
    yield SimpleNamespace(case=request.param, model=m, x=x, dy=dy, y=y, rec=rec, g_none=g_none)
    del m, rec, g_none
    torch.cuda.empty_cache()


def same(got, want, what):
    assert got is not None and want is not None, f"{what}: missing ({got is None}, {want is None})"
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError(f"{what}: not bit-identical ({int((d > 0).sum())} elements differ, max {float(d.max()):.3e})")


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ replay
def replay(node):
    """the node alone on its recorded inputs and incoming gradients with fresh leaves: (outputs, {slot: gradient})"""
    from py4cast_amd import ops_gemm as G
    from py4cast_amd import ops_rows as R
    from py4cast_amd import ops_ts as TS

    const = ("stats", "mul")        # (not differentiated: the producer's column sums, the dropout draw)
    a = {k: (None if v is None else v.clone().requires_grad_(k not in const)) for k, v in node.args.items()}
    extra = {}
    if node.kind == "bn":
        bn = copy.deepcopy(node.pre)
        o = node.opts
        out = G.batch_norm_act(a["y"], a["stats"], bn, o["slope"], a["res"], o["res_passthrough"], a["mul"], o["mul_factor"])
        outs = list(out) if o["res_passthrough"] else [out]
        extra = {"_bn": bn, "gamma": None, "beta": None}
    elif node.kind == "aln":
        outs = list(R.add_layer_norm(a["x"], a["add"], a["gamma"], a["beta"], node.eps))
    elif node.kind == "epa":
        outs = list(TS.epa_core(a["qkvv"], a["W"], a["bias"], a["t1"], a["t2"]))
    elif node.kind == "merge":
        outs = [TS.merge_published(a["x_sa"])]
    else:
        outs = [G.cat_linear_res(a["xa"], a["wa"], a["ba"], a["xb"], a["wb"], a["bb"], a["res"], gamma=a["gamma"])]
    pairs = [(o, g.clone()) for o, g in zip(outs, node.gout) if g is not None]
    torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs])
    torch.cuda.synchronize()        # (the deferred reductions of GradQueue are flushed when the backward pass ends)
    grads = {k: (None if a[k] is None else a[k].grad) for k in GRAD_SLOTS[node.kind] if k in a}
    if extra:
        grads.update(extra, gamma=extra["_bn"].weight.grad, beta=extra["_bn"].bias.grad)
    return [o.detach() for o in outs], grads


def test_replay_is_bit_identical(run):
    for i, node in enumerate(run.rec.nodes):
        outs, grads = replay(node)
        for j, (o, want) in enumerate(zip(outs, node.out)):
            same(o, want, f"node {i} {node.kind} out{j}")
        for slot, g in grads.items():
            if slot == "_bn":
                for k in ("running_mean", "running_var", "num_batches_tracked"):
                    same(getattr(g, k), getattr(node.post, k), f"node {i} bn {k}")
                continue
            want = node.grad(slot)
            if want is None and g is None:
                continue
            same(g, want, f"node {i} {node.kind} d{slot}")


# ------------------------------------------------------------------------------------------------ float64
def test_nodes_against_float64(run):
    worst = {}

    bad = []

    def bar(v, limit, what, key):
        worst[key] = max(worst.get(key, (0.0, limit)), (v, limit))
        if not v <= limit:
            bad.append(f"{what}: {v:.2e} > {limit:.0e}")

    def near(got, ref, what):
        got, ref = got.detach().double(), ref.detach().double()
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        bar(float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)), 6e-3, f"{what} (max)", "bf16 map, max")
        bar(rel(got, ref), 3e-3, f"{what} (2-norm)", "bf16 map, 2-norm")

    for i, node in enumerate(run.rec.nodes):
        outs, grads = replay(node)
        a, go, w = node.args, node.gout, f"node {i} {node.kind}"
        if node.kind == "aln":
            ref = UN.aln_node(a["x"], a["add"], a["gamma"], a["beta"], node.eps, t_stored=outs[0], dt=go[0], dln=go[1])
            near(outs[0], ref.t, f"{w} t")
            near(outs[1], ref.ln, f"{w} ln")
            near(grads["x"], ref.dx, f"{w} dx")
            bar(rel(grads["add"], ref.dadd), 5e-4, f"{w} dpos_embed", "aln dpos_embed")
            bar(rel(grads["gamma"], ref.dgamma), 5e-3, f"{w} dgamma", "aln dgamma, dbeta")
            bar(rel(grads["beta"], ref.dbeta), 5e-3, f"{w} dbeta", "aln dgamma, dbeta")
        elif node.kind == "epa":
            ref = UN.epa_node(a["qkvv"], a["W"], a["bias"], a["t1"], a["t2"], go[0], go[1])
            got = UN.epa_measure(*outs, grads["qkvv"], grads["W"], grads["bias"], grads["t1"], grads["t2"], ref)
            for q, v in got.items():
                bar(v, UN.EPA_BARS[q], f"{w} {q}", f"epa {q}")
        elif node.kind == "bn":
            o, pre, bn = node.opts, node.pre, grads["_bn"]
            kw = dict(res=a["res"], mul=a["mul"], factor=o["mul_factor"])
            own = UN.bn_act_node(a["y"], pre.weight, pre.bias, pre.eps, o["slope"], **kw)
            ref = UN.bn_act_node(a["y"], pre.weight, pre.bias, pre.eps, o["slope"], out_stored=outs[0], dout=go[0],
                                 dpass=go[1] if o["res_passthrough"] else None, **kw)
            near(outs[0], own.out, f"{w} out")        # against float64's own LeakyReLU decisions and the recorded dropout draw
            near(grads["y"], ref.dy, f"{w} dy")
            if a["res"] is not None:
                near(grads["res"], ref.dres, f"{w} dres (+ the passthrough gradient)")
                if o["res_passthrough"]:
                    same(outs[1], a["res"], f"{w} passthrough output (the residual itself)")
            bar(rel(grads["gamma"], ref.dgamma), 5e-3, f"{w} dgamma", "bn dgamma, dbeta")
            bar(rel(grads["beta"], ref.dbeta), 5e-3, f"{w} dbeta", "bn dgamma, dbeta")
            mo = pre.momentum
            bar(rel(bn.running_mean, (1 - mo) * pre.running_mean.double() + mo * ref.mean), 1e-4, f"{w} running_mean", "bn running")
            bar(rel(bn.running_var, (1 - mo) * pre.running_var.double() + mo * ref.var_unbiased), 1e-4, f"{w} running_var", "bn running")
            assert int(bn.num_batches_tracked) == int(pre.num_batches_tracked) + 1, f"{w} num_batches_tracked"
        elif node.kind == "merge":
            x_sa = a["x_sa"]
            B, H, N, d = x_sa.shape
            same(outs[0], UN.merge_published(x_sa), f"{w} out (the published permutation)")
            same(grads["x_sa"].contiguous(), go[0].reshape(B, d, H, N).permute(0, 2, 3, 1).contiguous(), f"{w} dx_sa (its inverse)")
        else:
            ref = UN.catlin_node(a["xa"], a["wa"], a["ba"], a["xb"], a["wb"], a["bb"], a["res"], a["gamma"], dy=go[0])
            near(outs[0], ref.y, f"{w} y")
            near(grads["xa"], ref.dxa, f"{w} dxa")
            near(grads["xb"], ref.dxb, f"{w} dxb")
            same(grads["res"], go[0], f"{w} dres (the incoming gradient itself)")
            for s, r64 in (("wa", ref.dwa), ("ba", ref.dba), ("wb", ref.dwb), ("bb", ref.dbb)):
                bar(rel(grads[s], r64), 5e-4, f"{w} d{s}", "catlin dW, db")
            bar(rel(grads["gamma"], ref.dgamma), 5e-3, f"{w} dgamma", "catlin dgamma")
        del outs, grads
    kinds = {k: sum(n.kind == k for n in run.rec.nodes) for k in GRAD_SLOTS}
    print(f"\n{run.case}: nodes {kinds}; worst value / bar:", ", ".join(f"{k} {v:.1e} / {lim:.0e}" for k, (v, lim) in sorted(worst.items())))
    assert not bad, "\n".join(bad[:40])


# ------------------------------------------------------------------------------------------------ wiring
def test_wiring_is_bit_identical(run):
    nodes, m = run.rec.nodes, run.model
    by_block, bns = {}, {}
    for n in nodes:
        by_block.setdefault(id(n.blk), {})[n.kind] = n
        if n.kind == "bn":
            bns.setdefault(id(n.blk), []).append(n)
    for blk in blocks(m):
        k = by_block[id(blk)]
        aln, cat, epa, mrg = k["aln"], k["catlin"], k.get("epa"), k.get("merge")
        same(aln.gout[0], cat.grad("res"), "aln t <- catlin dres")
        # conv51's two batch norms: norm1 plain; norm2 takes the skip as its residual, hands it on to conv8 (passthrough: conv8's
        # residual gradient must have reached this node) and applies the channel dropout's draw of the published block in training
        n1, n2 = bns[id(blk)]
        assert n1.module is blk.conv51.norm1 and n2.module is blk.conv51.norm2
        assert n1.args["res"] is None and n1.args["mul"] is None and not n1.opts["res_passthrough"]
        assert n2.args["res"] is not None and n2.opts["res_passthrough"] and n2.gout[1] is not None, "the skip's passthrough"
        p = blk.conv8[0].p if blk.published else 0.0
        if p > 0:
            mul = n2.args["mul"]
            assert mul is not None and mul.shape == (run.x.shape[0], blk.pos_embed.shape[-1]) and mul.dtype == torch.float32
            assert bool(((mul == 0) | (mul == 1)).all()) and n2.opts["mul_factor"] == 1.0 / (1.0 - p), "a Dropout2d draw per (sample, channel)"
        else:
            assert n2.args["mul"] is None
        if epa is None:
            continue
        B, H, N, d = epa.out[0].shape
        if mrg is not None:
            same(mrg.gout[0], cat.grad("xa"), "merge out <- catlin dxa")
            same(epa.gout[0], mrg.grad("x_sa"), "epa x_sa <- merge dx_sa")
        else:       # restated: the merge is a view of the token-major output
            same(epa.gout[0].permute(0, 2, 1, 3).reshape(B, N, H * d), cat.grad("xa"), "epa x_sa <- catlin dxa")
        same(epa.gout[1].permute(0, 2, 1, 3).reshape(B, N, H * d), cat.grad("xb"), "epa x_ca <- catlin dxb")
    # ownership: every parameter of these nodes belongs to one node; the network's p.grad is its replay gradient
    names = {id(p): n for n, p in m.named_parameters()}
    owner = {}
    for node in nodes:
        _, grads = replay(node)
        for slot, p in node.params().items():
            assert id(p) not in owner, f"{names[id(p)]}: taken by two nodes"
            owner[id(p)] = node.kind
            same(run.g_none[names[id(p)]], grads[slot], f"{names[id(p)]}: p.grad")
    # every parameter of a block whose attention runs on the node is owned, but those of the kinds not recorded here (the qkvv projection,
    # conv51's and conv8's convolutions)
    unrecorded = ("epa_block.qkvv.weight", "conv51.conv1.weight", "conv51.conv2.weight", "conv8.weight", "conv8.bias", "conv8.1.weight",
                  "conv8.1.bias")
    for blk in blocks(m):
        if "epa" in by_block[id(blk)]:
            for n, p in blk.named_parameters():
                assert n in unrecorded or id(p) in owner, f"{n}: no node owns it"
    # E = F (published block): one Linear under two names -- F is E, the state dict's F.* keys are E's tensors, and the ownership
    # above counted the parameter once
    for blk in blocks(m):
        e = blk.epa_block
        if e.published:
            assert e.F is e.E
            sd = e.state_dict()
            assert sd["F.weight"].data_ptr() == e.E.weight.data_ptr() and sd["F.bias"].data_ptr() == e.E.bias.data_ptr()
            assert sum(q is e.E.weight for q in e.parameters()) == 1


# ------------------------------------------------------------------------------------------------ sink route
def test_sink_route_adds_into_grad(run):
    from py4cast_amd.trainer import FlatDDP

    m = run.model
    g = torch.Generator(device=run.x.device).manual_seed(11)
    prefill = {n: (torch.rand(p.shape, device=p.device, generator=g) + 0.5) * (1 - 2 * (torch.rand(p.shape, device=p.device, generator=g) < 0.5))
               for n, p in m.named_parameters()}
    for n, p in m.named_parameters():
        p.grad = prefill[n].clone()
    y = step(m, run.x, run.dy)
    same(y, run.y, "rerun output (same draw)")
    for n, p in m.named_parameters():
        same(p.grad, prefill[n] + run.g_none[n], f"prefilled .grad: {n}")
    ddp = FlatDDP(m, 1)
    for n, p in m.named_parameters():
        assert p.grad.data_ptr() >= ddp.flat_grad.data_ptr(), n
        p.grad.copy_(prefill[n])
    step(m, run.x, run.dy)
    for n, p in m.named_parameters():
        same(p.grad, prefill[n] + run.g_none[n], f"FlatDDP .grad: {n}")
