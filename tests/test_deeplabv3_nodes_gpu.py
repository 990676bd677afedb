"""
DeepLabV3 (py4cast_amd/deeplabv3.py) node by node: one forward / backward of DeepLabV3MI355X's bf16 route under tests/deeplabv3_nodes.py's
recorder, then for every recorded node (the strided patch convolutions, the implicit-GEMM convolutions with their dilation / passthrough /
bias, the batch norms with their residual and Dropout multiplier, the stem tail, the ASPP assembly, the x8 up-sampling):

* replay: the node alone on its recorded inputs and incoming gradient, with fresh parameter leaves, gives the in-network outputs and
  input / parameter gradients BIT FOR BIT (every native reduction has a fixed order), the stem's routing table included;
* float64: the replay against the float64 node reference -- forward outputs against the reference's own decisions (an output wrongly
  left at zero shows), gradients with every decision (ReLU mask, the Dropout draw = model.last_dropout_mask, the stem's max-pool
  routing = the ``arg`` table _StemTail saved) taken from the device -- so no gradient comparison crosses a decision and the bars are the
  kernel tests' (tests/test_gemm_gpu.py, tests/test_unet_nodes_gpu.py): bf16 maps <= 6e-3 of the largest magnitude per element and
  <= 3e-3 in the 2-norm; convolution weight / bias gradients <= 5e-4, 3e-3 for the dilated 3x3 ones (test_dilated_conv_against_float64:
  the dilated weight-gradient kernel sums bf16 products of taps far apart); batch-norm gamma / beta gradients <= 5e-3 (3e-3 for the stem
  tail, its kernel test's bar); running mean / var <= 1e-4 with num_batches_tracked advanced by exactly one; plus an eval-mode forward
  of every batch norm on the running statistics the training call left;
* wiring: the gradient each node's output received is its consumer's input gradient -- bit for bit where there is one consumer
  (including the identity edge of a residual block, whose gradient conv1's passthrough adds inside its data-gradient launch), and where
  autograd sums several (the input of layer2.0 / layer3.0 / layer4.0: conv1 and the downsample; the ASPP input: four convolutions and
  the pooling branch) equal to their float64 sum within the bf16 roundings of those adds; every parameter belongs to exactly one node
  and the network's p.grad is that node replay's gradient;
* sink route: the same backward with every .grad pre-filled, and under FlatDDP with a non-zero flat buffer: p.grad = prefill + the
  gradient of the first run, bit for bit (the stem's batch norm through p4c_inorm_finalize_bwd, the ASPP pooling head, the patch
  convolutions' weights and the head's padded weight and bias through autograd's accumulation, the rest through the GEMM's sink).

The ASPP pooling branch's batch norm at B = 2: with two values per channel the normalised output is +-1 whatever z is, so every
gradient through it (the branch's dx and 1x1 weight gradient) is driven by eps alone and a relative bar on it measures cancellation.
The B = 3 toy case holds that node to the ordinary bars.  At B = 2 its dx and weight-gradient errors are bounded relative to the scale
of the gradients around the cancellation -- the size they would have without it, |gamma| rstd |dpooled| carried through the 1x1 weight
and the 1 / HW broadcast (dx: 6e-3 of the largest) or against the sample means (dw: 5e-4 in the 2-norm); gamma / beta, whose gradients
do not cancel, keep the ordinary bars.

Measured at the benchmark size (2 x 512 x 512, 69 -> 60 channels, resnet18, dc = 256, Dropout 0.5; worst node / bar): bf16 maps
4.2e-3 / 6e-3 per element and 2.3e-3 / 3e-3 in the 2-norm (bf16 rounding of the stored maps), convolution weight / bias gradients
7.8e-7 / 5e-4, dilated 3x3 weight gradients 6.6e-7 / 3e-3, BN gamma / beta gradients 3.6e-6 / 5e-3, stem tail 3.6e-7 / 3e-3, running
mean / var 2.9e-7 / 1e-4, statistics epilogues 4.2e-8 / 1e-5; the ASPP pooling branch at B = 2: dx 4.0e-4 / 6e-3 and dw 6.8e-6 / 5e-4
of their scales (the B = 3 toy case: within the ordinary bars).  The whole file takes about 20 s on one MI355X.
"""
import copy
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deeplabv3_nodes as N  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (B, H, W, in_channels, out_channels, encoder, decoder_channels, aspp_dropout)
CASES = {
    "toy-r18-p0": (2, 64, 64, 69, 60, "resnet18", 64, 0.0),
    "toy-r18-p05": (2, 64, 64, 69, 60, "resnet18", 64, 0.5),
    "toy-r34-64x96": (2, 64, 96, 69, 60, "resnet34", 64, 0.0),
    "toy-r18-b3": (3, 64, 64, 69, 60, "resnet18", 64, 0.0),
    "bench": (2, 512, 512, 69, 60, "resnet18", 256, 0.5),     # bench.py --model DeepLabV3: 69 input channels -> 72, Dropout 0.5
    "titan": (2, 512, 640, 46, 21, "resnet18", 256, 0.5),     # the Titan grid; 46 input channels -> 48
}
SEED = 5        # the generator state every forward starts from (the Dropout draw)


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def same(got, want, what):
    assert got is not None and want is not None, f"{what}: missing ({got is None}, {want is None})"
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError(f"{what}: not bit-identical ({int((d > 0).sum())} elements differ, max {float(d.max()):.3e})")


def to_param(g, p):
    """a node's gradient of the (padded) operand it was given, as the parameter's own shape (the head's zero output rows sliced off)"""
    return g[tuple(slice(0, s) for s in p.shape)]


def make_model(case, dev):
    from py4cast_amd.deeplabv3 import DeepLabV3MI355X, DeepLabV3Settings

    B, H, W, cin, cout, enc, dc, p = CASES[case]
    torch.manual_seed(0)
    m = DeepLabV3MI355X(cin, cout, (H, W), DeepLabV3Settings(encoder_name=enc, decoder_channels=dc, encoder_weights=False, aspp_dropout=p,
                                                             compute_dtype="bf16", activation_dtype="bf16")).to(dev).train()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.3, 0.3)
            elif getattr(mod, "bias", None) is not None:
                mod.bias.uniform_(-0.3, 0.3)
    g = torch.Generator(device=dev).manual_seed(7)
    # spread per-sample inputs (tests/test_deeplabv3_gpu.py::_inputs): the pooling branch's batch norm over the B sample means
    x = torch.randn(B, H, W, cin, device=dev, generator=g)
    for b in range(B):
        x[b] = x[b] * (1.0 + b) + 0.5 * b
    dy = torch.randn(B, H, W, cout, device=dev, generator=g)
    return m, x, dy


def step(m, x, dy):
    torch.manual_seed(SEED)
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    y.float().backward(dy)
    torch.cuda.synchronize()
    return y.detach(), xg.grad


@pytest.fixture(scope="module", params=list(CASES))
def run(request, gpu_device):
    torch.cuda.empty_cache()
    m, x, dy = make_model(request.param, gpu_device)
    with N.Recorder(m) as rec:
        y, dx = step(m, x, dy)
    for n in rec.nodes:
        assert n.gout is not None and n.gin is not None, f"{n.name}: no backward recorded"
    g_none = {name: p.grad.detach().clone() for name, p in m.named_parameters()}
    mask = None if m.last_dropout_mask is None else m.last_dropout_mask.clone()
    ns = SimpleNamespace(case=request.param, model=m, x=x, dy=dy, y=y, dx=dx, rec=rec, g_none=g_none, mask=mask, B=x.shape[0], _replays=None)
    yield ns
    del m, rec, g_none, ns
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ replay
def _fresh(t):
    return None if t is None else t.clone().requires_grad_(True)


def replay(node):
    """the node alone on its recorded inputs, its recorded incoming gradient and fresh parameter leaves: (outputs, {slot: gradient},
    the node's batch norm after the call or None, the stem's routing table or None)"""
    from py4cast_amd import deeplabv3 as D
    from py4cast_amd import ops_gemm as G

    a, o = node.args, node.opts
    bn = arg = None
    if node.kind == "patch":
        x, w = _fresh(a["x"]), _fresh(a["w"])
        k, s, p = o["k"], o["stride"], o["pad"]
        conv = SimpleNamespace(weight=w, kernel_size=(k, k), stride=(s, s), padding=(p, p))
        outs = list(D.DeepLabV3MI355X._patch(conv, x))
        outs[0].backward(node.gout[0].clone())
        grads = {"x": x.grad, "w": w.grad}
    elif node.kind == "conv":
        x, w, b = _fresh(a["x"]), _fresh(a["w"]), _fresh(a["b"])
        out = G.conv2d_nhwc(x, w, b, want_stats=o["want_stats"], passthrough=o["passthrough"], dilation=o["dilation"])
        out = list(out) if isinstance(out, tuple) else [out]
        outs = [out[0], out[1] if o["want_stats"] else None, out[-1] if o["passthrough"] else None]
        pairs = [(t, g.clone()) for t, g in zip(outs, node.gout) if t is not None and g is not None]
        torch.autograd.backward([q[0] for q in pairs], [q[1] for q in pairs])
        grads = {"x": x.grad, "w": w.grad, "b": None if b is None else b.grad}
    elif node.kind == "bn":
        bn = copy.deepcopy(node.pre)
        bn.weight.grad = bn.bias.grad = None
        y, res = _fresh(a["y"]), _fresh(a["res"])
        st = None if a["stats"] is None else a["stats"].clone()
        mul = None if a["mul"] is None else a["mul"].clone()
        outs = [G.batch_norm_act(y, st, bn, slope=o["slope"], res=res, mul=mul, mul_factor=o["mul_factor"])]
        outs[0].backward(node.gout[0].clone())
        grads = {"y": y.grad, "gamma": bn.weight.grad, "beta": bn.bias.grad, "res": None if res is None else res.grad}
    elif node.kind == "stem":
        bn = copy.deepcopy(node.pre)
        bn.weight.grad = bn.bias.grad = None
        y = _fresh(a["y"])
        outs = [D.stem_tail(y, None if a["stats"] is None else a["stats"].clone(), bn)]
        arg = outs[0].grad_fn.saved_tensors[2].clone()
        outs[0].backward(node.gout[0].clone())
        grads = {"y": y.grad, "gamma": bn.weight.grad, "beta": bn.bias.grad}
    elif node.kind == "aspp":
        pb = copy.deepcopy(node.module)
        pb[2] = copy.deepcopy(node.pre)
        for q in pb.parameters():
            q.grad = None
        bn = pb[2]
        x = _fresh(a["x"])
        br = [_fresh(a[f"a{k}"]) for k in range(4)]
        outs = [D.aspp_assemble(x, br, pb)]
        outs[0].backward(node.gout[0].clone())
        grads = {"x": x.grad, **{f"a{k}": br[k].grad for k in range(4)}, "w": pb[1].weight.grad, "gamma": bn.weight.grad, "beta": bn.bias.grad}
    else:
        x = _fresh(a["x"])
        outs = [D.upsample_bilinear_ac(x, o["scale"])]
        outs[0].backward(node.gout[0].clone())
        grads = {"x": x.grad}
    torch.cuda.synchronize()
    return [None if t is None else t.detach() for t in outs], grads, bn, arg


def replays(run):
    if run._replays is None:
        run._replays = [replay(n) for n in run.rec.nodes]
    return run._replays


def node_grad(node, slot):
    """the recorded backward result for `slot`, as the shape of the operand the replay's leaf has (the patch convolution's (Co, C k^2)
    weight gradient of the padded weight -> the parameter's (Co, Ci, k, k))"""
    g = node.grad(slot)
    if node.kind == "patch" and slot == "w" and g is not None:
        k, Ci = node.opts["k"], node.args["w"].shape[1]
        g = g.view(g.shape[0], -1, k, k)[:, :Ci]
    return g


def test_replay_is_bit_identical(run):
    for node, (outs, grads, bn, arg) in zip(run.rec.nodes, replays(run)):
        for j, (o, want) in enumerate(zip(outs, node.out)):
            if want is None:
                continue
            same(o, want, f"{node.name} out{j}")
        for slot, g in grads.items():
            want = node_grad(node, slot)
            if want is None and g is None:
                continue
            same(g, want, f"{node.name} d{slot}")
        if node.kind == "stem":
            same(arg, node.saved["arg"], f"{node.name} routing table")
        if bn is not None:
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                same(getattr(bn, k), getattr(node.post, k), f"{node.name} {k}")


# ------------------------------------------------------------------------------------------------ float64
def test_nodes_against_float64(run):
    """every node's replay against its float64 reference (decisions from the stored values); prints the worst value met per bar"""
    from py4cast_amd import deeplabv3 as D
    from py4cast_amd import ops_gemm as G

    worst = {}
    rec = run.rec

    def bar(v, limit, what, key):
        worst[key] = max(worst.get(key, (0.0, limit)), (v, limit))
        assert v <= limit, f"{what}: {v:.2e} > {limit:.0e}"

    def near(got, ref, what):
        got, ref = got.detach().double(), ref.detach().double()
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        bar(float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)), 6e-3, f"{what} (max)", "bf16 map, max")
        bar(rel(got, ref), 3e-3, f"{what} (2-norm)", "bf16 map, 2-norm")

    def stats_epilogue(y, st, what):
        # the statistics epilogue: column sums of the ROUNDED output (test_dilated_conv_against_float64)
        s = st.double().sum(0)
        yr = y.double().reshape(-1, y.shape[-1])
        bar(max(rel(s[0], yr.sum(0)), rel(s[1], (yr * yr).sum(0))), 1e-5, f"{what} stats", "stats epilogue")

    def norm_checks(node, pre, bn, ref, gbar):
        for slot, r64 in (("gamma", ref.dgamma), ("beta", ref.dbeta)):
            bar(rel(grads[slot], r64), gbar, f"{node.name} d{slot}", "BN dgamma, dbeta" if gbar == 5e-3 else "stem dgamma, dbeta")
        rm, rv = N.running_update(pre, ref, pre.momentum)
        bar(rel(bn.running_mean, rm), 1e-4, f"{node.name} running_mean", "running mean, var")
        bar(rel(bn.running_var, rv), 1e-4, f"{node.name} running_var", "running mean, var")
        assert int(bn.num_batches_tracked) == int(pre.num_batches_tracked) + 1, f"{node.name} num_batches_tracked"

    for node, (outs, grads, bn, arg) in zip(rec.nodes, replays(run)):
        a, o, go, pre = node.args, node.opts, node.gout, node.pre
        if node.kind == "patch":
            y64, dx64, dw64, _ = N.conv_node(a["x"], a["w"], stride=o["stride"], pad=o["pad"], dy=go[0])
            near(outs[0], y64, f"{node.name} y")
            stats_epilogue(outs[0], outs[1], node.name)
            near(grads["x"], dx64, f"{node.name} dx")
            bar(rel(grads["w"], dw64), 5e-4, f"{node.name} dw", "conv dw, db")
        elif node.kind == "conv":
            d, k = o["dilation"], a["w"].shape[2]
            y64, dx64, dw64, db64 = N.conv_node(a["x"], a["w"], a["b"], pad=d if k == 3 else 0, dilation=d, dy=go[0])
            near(outs[0], y64, f"{node.name} y")
            if o["want_stats"]:
                stats_epilogue(outs[0], outs[1], node.name)
            if o["passthrough"]:
                same(outs[2], a["x"], f"{node.name} passthrough")
                dx64 = dx64 + go[2].double()          # the residual's gradient, added in the data gradient's epilogue
            near(grads["x"], dx64, f"{node.name} dx")
            wb = 3e-3 if d > 1 else 5e-4
            bar(rel(grads["w"], dw64), wb, f"{node.name} dw", "conv dw, db" if d == 1 else "dilated conv dw")
            if db64 is not None:
                bar(rel(grads["b"], db64), 5e-4, f"{node.name} db", "conv dw, db")
        elif node.kind == "bn":
            if a["mul"] is not None:
                same(a["mul"], run.mask, f"{node.name} multiplier = model.last_dropout_mask")
                p = run.model.decoder[0].project[3].p
                assert o["mul_factor"] == pytest.approx(1.0 / (1.0 - p), rel=1e-7), f"{node.name} mul_factor"
            kw = dict(slope=o["slope"], res=a["res"], mul=a["mul"], factor=o["mul_factor"])
            own = N.bn_act(a["y"], pre.weight, pre.bias, pre.eps, **kw)
            ref = N.bn_act(a["y"], pre.weight, pre.bias, pre.eps, mask=outs[0] > 0, dout=go[0], **kw)
            # the forward against float64's OWN ReLU (an output wrongly left at zero must show); the backward on the stored decisions
            near(outs[0], own.out, f"{node.name} out")
            near(grads["y"], ref.dy, f"{node.name} dy")
            if a["res"] is not None:
                near(grads["res"], ref.dres, f"{node.name} dres")
            norm_checks(node, pre, bn, ref, 5e-3)
            bn.eval()
            with torch.no_grad():
                oe = G.batch_norm_act(a["y"], None, bn, slope=o["slope"], res=a["res"])
            re_ = N.bn_act(a["y"], bn.weight, bn.bias, bn.eps, slope=o["slope"], res=a["res"], running=(bn.running_mean, bn.running_var))
            near(oe, re_.out, f"{node.name} eval out")
        elif node.kind == "stem":
            assert int(arg.max()) <= 8
            ref = N.stem_node(a["y"], pre.weight, pre.bias, pre.eps, arg=arg, pool_stored=outs[0], dpool=go[0])
            near(outs[0], ref.pool, f"{node.name} pool")                 # on float64's own maxima
            near(outs[0], ref.pool_at_arg, f"{node.name} pool at arg")   # the device's choice is a maximum, to rounding
            near(grads["y"], ref.dy, f"{node.name} dy")
            norm_checks(node, pre, bn, ref, 3e-3)
            bn.eval()
            with torch.no_grad():
                pe = D.stem_tail(a["y"], None, bn)
            near(pe, N.stem_node(a["y"], bn.weight, bn.bias, bn.eps, running=(bn.running_mean, bn.running_var)).pool, f"{node.name} eval pool")
        elif node.kind == "aspp":
            Dd = a["w"].shape[0]
            br = [a[f"a{k}"] for k in range(4)]
            for k in range(4):
                same(outs[0][..., k * Dd: (k + 1) * Dd], br[k], f"{node.name} branch {k}")
                same(grads[f"a{k}"], go[0][..., k * Dd: (k + 1) * Dd], f"{node.name} da{k}")
            pooled = outs[0][:, 0, 0, 4 * Dd:]
            assert torch.equal(outs[0][..., 4 * Dd:], pooled[:, None, None, :].expand_as(outs[0][..., 4 * Dd:])), f"{node.name} broadcast"
            ref = N.aspp_node(a["x"], br, a["w"], pre.weight, pre.bias, pre.eps, pooled_stored=pooled, dbuf=go[0])
            near(pooled, ref.pooled, f"{node.name} pooled")
            if run.B >= 3:
                near(grads["x"], ref.dx, f"{node.name} dx")
                bar(rel(grads["w"], ref.dw), 5e-4, f"{node.name} dw", "conv dw, db")
            else:
                # B = 2: the branch's gradients are eps-driven (module docstring) -- their errors bounded relative to the size the same
                # gradients would have without the batch norm's cancellation, |gamma| rstd |dpooled| carried through the 1x1 weight
                # (dx: and the 1 / HW broadcast) or against the sample means (dw)
                u = pre.weight.detach().double().abs() * torch.rsqrt(ref.var + pre.eps) * go[0][..., 4 * Dd:].double().sum((1, 2)).abs()
                xm = a["x"].double().mean((1, 2)).abs()
                s_dx = (u @ a["w"].detach().double().reshape(Dd, -1).abs()) / (a["x"].shape[1] * a["x"].shape[2])
                s_dw = u.t() @ xm
                bar(float((grads["x"].double() - ref.dx).abs().max() / s_dx.max()), 6e-3, f"{node.name} dx (B = 2)", "ASPP pool B=2 dx / scale")
                err_dw = grads["w"].double().reshape(s_dw.shape) - ref.dw.reshape(s_dw.shape)
                bar(float(err_dw.norm() / s_dw.norm()), 5e-4, f"{node.name} dw (B = 2)", "ASPP pool B=2 dw / scale")
            norm_checks(node, pre, bn, ref, 5e-3)
            pb = copy.deepcopy(node.module)
            pb[2] = bn
            pb.eval()
            with torch.no_grad():
                be = D.aspp_assemble(a["x"], br, pb)
            re_ = N.aspp_node(a["x"], br, a["w"], bn.weight, bn.bias, bn.eps, running=(bn.running_mean, bn.running_var))
            near(be[:, 0, 0, 4 * Dd:], re_.pooled, f"{node.name} eval pooled")
        else:
            up64, dx64 = N.upsample_node(a["x"], o["scale"], dout=go[0])
            near(outs[0], up64, f"{node.name} up")
            near(grads["x"], dx64, f"{node.name} dx")
    print(f"\n{run.case}: worst value / bar:", ", ".join(f"{k} {v:.1e} / {lim:.0e}" for k, (v, lim) in sorted(worst.items())))


# ------------------------------------------------------------------------------------------------ wiring
def test_wiring(run):
    rec, m = run.rec, run.model
    nodes = rec.nodes
    consumers, unmatched = {}, []
    for node in nodes:
        for slot in N.DIFF_INPUTS[node.kind]:
            if node.args.get(slot) is None:
                continue
            if slot in node.src:
                consumers.setdefault(node.src[slot], []).append((node, slot))
            else:
                unmatched.append(f"{node.name} {slot}")
    # every node input but the network's own is a recorded output: a model change that puts a copy between two nodes must fail here,
    # not drop the edge from the checks below
    assert unmatched == ["encoder.conv1 x"], f"node inputs not traced to a recorded output: {unmatched}"
    multi = {}
    for (j, o), cons in consumers.items():
        got = nodes[j].gout[o]
        if len(cons) == 1:
            node, slot = cons[0]
            same(got, node.grad(slot), f"{node.name} d{slot} -> {nodes[j].name} out{o}")
            continue
        multi[nodes[j].name] = sorted(f"{n.name} {s}" for n, s in cons)
        # autograd sums the consumers' bf16 gradients, rounding after each add: within (k - 1) half-ulps of the running sums
        terms = [n.grad(s).double() for n, s in cons]
        exact = sum(terms)
        slack = (len(terms) - 1) * 2.0 ** -8 * sum(t.abs() for t in terms)
        err = (got.double() - exact).abs()
        assert bool((err <= slack).all()), f"{nodes[j].name} out{o}: gradient is not the sum of its {len(cons)} consumers' (max excess {float((err - slack).max()):.3e})"
    enc = m.encoder
    last = {li: f"encoder.layer{li}.{len(getattr(enc, f'layer{li}')) - 1}.bn2" for li in (1, 2, 3, 4)}
    want = {last[1]: ["encoder.layer2.0.conv1 x", "encoder.layer2.0.downsample.0 x"],
            last[2]: ["encoder.layer3.0.conv1 x", "encoder.layer3.0.downsample.0 x"],
            last[3]: ["encoder.layer4.0.conv1 x", "encoder.layer4.0.downsample.0 x"],
            last[4]: sorted([f"decoder.0.convs.{k}.0 x" for k in range(4)] + ["decoder.0.convs.4 x"])}
    assert multi == want, multi
    # the identity edges: each residual batch norm's res is conv1's passthrough output (no downsample) or the downsample's norm
    for node in nodes:
        if node.kind == "bn" and node.args["res"] is not None:
            j, o = node.src["res"]
            blk = node.name.rsplit(".", 1)[0]
            assert (nodes[j].name, o) in ((f"{blk}.conv1", 2), (f"{blk}.downsample.1", 0)), (node.name, nodes[j].name, o)
    up = rec["segmentation_head.1"]
    cout = m.out_channels
    same(up.gout[0][..., :cout], run.dy.to(torch.bfloat16), "up-sampling dy")
    assert not up.gout[0][..., cout:].any(), "up-sampling dy: the padded output channels"
    same(rec["encoder.conv1"].grad("x")[..., :m.in_channels].float(), run.dx, "encoder.conv1 dx (the network's input gradient)")


def test_parameter_gradients_are_the_node_replays(run):
    m = run.model
    names = {id(p): n for n, p in m.named_parameters()}
    owner = {}
    for node, (_, grads, _, _) in zip(run.rec.nodes, replays(run)):
        for slot, p in node.params().items():
            assert id(p) not in owner, f"{node.name} {slot}: parameter already taken by {owner[id(p)]}"
            owner[id(p)] = node.name
            same(run.g_none[names[id(p)]], to_param(grads[slot], p).to(p.dtype), f"{node.name} {slot}: p.grad")
    for name, p in m.named_parameters():
        assert id(p) in owner, f"{name}: no node owns it"


# ------------------------------------------------------------------------------------------------ sink route
def test_sink_route_adds_into_grad(run):
    """p.grad pre-filled, and under FlatDDP (every .grad a view of one non-zero flat buffer, as bench.py builds it): p.grad = prefill +
    the gradient of the .grad-is-None run, bit for bit (same generator state: the same Dropout draw)"""
    from py4cast_amd.trainer import FlatDDP

    m = run.model
    g = torch.Generator(device=run.x.device).manual_seed(11)
    prefill = {n: (torch.rand(p.shape, device=p.device, generator=g) + 0.5) * (1 - 2 * (torch.rand(p.shape, device=p.device, generator=g) < 0.5))
               for n, p in m.named_parameters()}
    for n, p in m.named_parameters():
        p.grad = prefill[n].clone()
    step(m, run.x, run.dy)
    if run.mask is not None:
        same(m.last_dropout_mask, run.mask, "the Dropout draw of the rerun")
    for n, p in m.named_parameters():
        same(p.grad, prefill[n] + run.g_none[n], f"prefilled .grad: {n}")
    ddp = FlatDDP(m, 1)
    for n, p in m.named_parameters():
        assert p.grad.data_ptr() >= ddp.flat_grad.data_ptr(), n
        p.grad.copy_(prefill[n])
    step(m, run.x, run.dy)
    for n, p in m.named_parameters():
        same(p.grad, prefill[n] + run.g_none[n], f"FlatDDP .grad: {n}")
