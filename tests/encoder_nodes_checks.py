"""
What tests/test_customunet_nodes_gpu.py and tests/test_deeplabv3plus_nodes_gpu.py share: the five checks of
tests/test_deeplabv3_nodes_gpu.py (its module docstring states them and derives the bars) over the node kinds of
tests/deeplabv3_nodes.py, tests/customunet_nodes.py and tests/deeplabv3plus_nodes.py.  ``run`` is the namespace a test module's fixture
builds from one recorded forward / backward: case, model, x, dy, y, dx, rec, g_none, mask, B, dropout_p, step (the function that reruns
the step from the same generator state).

Bars (none is new): bf16 maps <= 6e-3 of the largest magnitude per element and <= 3e-3 in the 2-norm; convolution weight / bias
gradients <= 5e-4, 3e-3 for the dilated 3x3 ones; BN gamma / beta gradients <= 5e-3, 3e-3 for the stem tail; running statistics <= 1e-4;
statistics epilogue <= 1e-5; depthwise weight gradients <= 5e-4 (test_depthwise_dilated_against_float64); moved values bit-exact (the
skip channels and dskip of upcat, the forward and dskip of up2cat, the gradient up2into hands on, the zeros of pad channels); up2cat /
up2into dx within 2^-8 |sum| + 2^-22 sum|terms| of the float64 sum of the four (tests/test_customunet_gpu.py::_check_dx; reported as
the worst error over that bound); upcat's up-sampled channels and da equal upsample_bilinear_ac and its backward bit for bit.
"""
import copy
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import deeplabv3_nodes as N

STEMS = ("stem", "stemskip")


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


def randomise(m):
    """BN gamma / beta and every bias off their initial 1 / 0 / 0"""
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.3, 0.3)
            elif getattr(mod, "bias", None) is not None:
                mod.bias.uniform_(-0.3, 0.3)


def inputs(B, H, W, cin, cout, dev):
    """spread per-sample inputs x[b] * (1 + b) + 0.5 b (tests/test_deeplabv3_gpu.py::_inputs) and the output gradient"""
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(B, H, W, cin, device=dev, generator=g)
    for b in range(B):
        x[b] = x[b] * (1.0 + b) + 0.5 * b
    return x, torch.randn(B, H, W, cout, device=dev, generator=g)


def record(case, m, x, dy, recorder, seed, dropout_p=0.0):
    """one recorded forward / backward of m: the namespace the five checks read"""

    def step(m, x, dy):
        torch.manual_seed(seed)
        xg = x.clone().requires_grad_(True)
        y = m(xg)
        y.float().backward(dy)
        torch.cuda.synchronize()
        return y.detach(), xg.grad

    with recorder(m) as rec:
        y, dx = step(m, x, dy)
    for n in rec.nodes:
        assert n.gout is not None and n.gin is not None, f"{n.name}: no backward recorded"
    g_none = {name: p.grad.detach().clone() for name, p in m.named_parameters()}
    mask = getattr(m, "last_dropout_mask", None)
    mask = None if mask is None else mask.clone()
    return SimpleNamespace(case=case, model=m, x=x, dy=dy, y=y, dx=dx, rec=rec, g_none=g_none, mask=mask, B=x.shape[0], dropout_p=dropout_p,
                           step=step, _replays=None)


# ------------------------------------------------------------------------------------------------ replay
def _fresh(t):
    return None if t is None else t.clone().requires_grad_(True)


def replay(node, gout=None):
    """the node alone on its recorded inputs, its recorded incoming gradients (or `gout`) and fresh parameter leaves: (outputs,
    {slot: gradient}, the node's batch norm after the call or None, the stem's routing table or None)"""
    from py4cast_amd import customunet as U
    from py4cast_amd import deeplabv3 as D
    from py4cast_amd import deeplabv3plus as DP
    from py4cast_amd import ops_gemm as G

    a, o = node.args, node.opts
    gout = node.gout if gout is None else gout
    bn = arg = None

    def own_norm():
        bn = copy.deepcopy(node.pre)
        bn.weight.grad = bn.bias.grad = None
        return bn

    if node.kind == "patch":
        x, w = _fresh(a["x"]), _fresh(a["w"])
        k, s, p = o["k"], o["stride"], o["pad"]
        conv = SimpleNamespace(weight=w, kernel_size=(k, k), stride=(s, s), padding=(p, p))
        outs = list(D.DeepLabV3MI355X._patch(conv, x))
        outs[0].backward(gout[0].clone())
        grads = {"x": x.grad, "w": w.grad}
    elif node.kind == "conv":
        x, w, b = _fresh(a["x"]), _fresh(a["w"]), _fresh(a["b"])
        out = G.conv2d_nhwc(x, w, b, want_stats=o["want_stats"], passthrough=o["passthrough"], dilation=o["dilation"])
        out = list(out) if isinstance(out, tuple) else [out]
        outs = [out[0], out[1] if o["want_stats"] else None, out[-1] if o["passthrough"] else None]
        pairs = [(t, g.clone()) for t, g in zip(outs, gout) if t is not None and g is not None]
        torch.autograd.backward([q[0] for q in pairs], [q[1] for q in pairs])
        grads = {"x": x.grad, "w": w.grad, "b": None if b is None else b.grad}
    elif node.kind == "bn":
        bn = own_norm()
        y, res = _fresh(a["y"]), _fresh(a["res"])
        st = None if a["stats"] is None else a["stats"].clone()
        mul = None if a["mul"] is None else a["mul"].clone()
        outs = [G.batch_norm_act(y, st, bn, slope=o["slope"], res=res, mul=mul, mul_factor=o["mul_factor"])]
        outs[0].backward(gout[0].clone())
        grads = {"y": y.grad, "gamma": bn.weight.grad, "beta": bn.bias.grad, "res": None if res is None else res.grad}
    elif node.kind == "stem":
        bn = own_norm()
        y = _fresh(a["y"])
        outs = [D.stem_tail(y, None if a["stats"] is None else a["stats"].clone(), bn)]
        arg = outs[0].grad_fn.saved_tensors[2].clone()
        outs[0].backward(gout[0].clone())
        grads = {"y": y.grad, "gamma": bn.weight.grad, "beta": bn.bias.grad}
    elif node.kind == "stemskip":
        bn = own_norm()
        y = _fresh(a["y"])
        outs = list(U.stem_tail_skip(y, None if a["stats"] is None else a["stats"].clone(), bn, o["offset"]))
        arg = outs[1].grad_fn.saved_tensors[2].clone()
        torch.autograd.backward(outs, [gout[0].clone(), gout[1].clone()])
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
        outs[0].backward(gout[0].clone())
        grads = {"x": x.grad, **{f"a{k}": br[k].grad for k in range(4)}, "w": pb[1].weight.grad, "gamma": bn.weight.grad, "beta": bn.bias.grad}
    elif node.kind == "dw":
        R = len(o["rates"])
        x = _fresh(a["x"])
        ws = [_fresh(a[f"w{r}"]) for r in range(R)]
        outs = list(DP.depthwise3x3_dilated(x, ws, o["rates"]))       # R = 3: ONE three-rate call, as in the network
        torch.autograd.backward(outs, [g.clone() for g in gout])
        grads = {"x": x.grad, **{f"w{r}": ws[r].grad for r in range(R)}}
    elif node.kind == "upcat":
        x, skip = _fresh(a["a"]), _fresh(a["skip"])
        outs = [DP.up_cat(x, skip, o["scale"], o["ld"])]
        outs[0].backward(gout[0].clone())
        grads = {"a": x.grad, "skip": skip.grad}
    elif node.kind == "up2cat":
        x, skip = _fresh(a["x"]), _fresh(a["skip"])
        outs = [U.up2_cat(x, skip)]
        outs[0].backward(gout[0].clone())
        grads = {"x": x.grad, "skip": None if skip is None else skip.grad}
    elif node.kind == "up2into":
        x, base = _fresh(a["x"]), _fresh(a["buf"])     # from a copy of the recorded buffer (f1 beside uninitialised channels)
        outs = [U.up2_into(x, base.clone())]           # (a non-leaf the in-place node may write)
        outs[0].backward(gout[0].clone())
        grads = {"x": x.grad, "buf": base.grad}
    else:
        assert node.kind == "up", node.kind
        x = _fresh(a["x"])
        outs = [D.upsample_bilinear_ac(x, o["scale"])]
        outs[0].backward(gout[0].clone())
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


def defined(node, j, t):
    """output j of a node where it is defined: the stem-with-skip's buffer from its channel offset on (the channels before it are
    uninitialised until up2_into fills them)"""
    return t[..., node.opts["offset"]:] if (node.kind == "stemskip" and j == 0) else t


def check_replay_is_bit_identical(run):
    for node, (outs, grads, bn, arg) in zip(run.rec.nodes, replays(run)):
        for j, (o, want) in enumerate(zip(outs, node.out)):
            if want is None:
                continue
            same(defined(node, j, o), defined(node, j, want), f"{node.name} out{j}")
        for slot, g in grads.items():
            want = node_grad(node, slot)
            if want is None and g is None:
                continue
            same(g, want, f"{node.name} d{slot}")
        if node.kind in STEMS:
            same(arg, node.saved["arg"], f"{node.name} routing table")
        if bn is not None:
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                same(getattr(bn, k), getattr(node.post, k), f"{node.name} {k}")


# ------------------------------------------------------------------------------------------------ float64
def check_nodes_against_float64(run):
    """every node's replay against its float64 reference (decisions from the stored values); prints and returns the worst value met
    per bar"""
    from py4cast_amd import customunet as U
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

    def sum_of_four(dx, dout, Cx, what):
        # tests/test_customunet_gpu.py::_check_dx: half a bf16 ulp of the sum + the three fp32 additions
        B, H2, W2, _ = dout.shape
        d = dout[..., :Cx].double().view(B, H2 // 2, 2, W2 // 2, 2, Cx)
        s, mag = d.sum(dim=(2, 4)), d.abs().sum(dim=(2, 4))
        bound = 2.0 ** -8 * s.abs() + 2.0 ** -22 * mag
        err = (dx.double() - s).abs()
        live = bound > 0
        assert bool((err[~live] == 0).all()), f"{what}: a sum of four zeros is not zero"
        bar(float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0, 1.0, what, "up2cat dx / its bound")

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
                assert o["mul_factor"] == pytest.approx(1.0 / (1.0 - run.dropout_p), rel=1e-7), f"{node.name} mul_factor"
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
        elif node.kind == "stemskip":
            off = o["offset"]
            assert int(arg.max()) <= 8
            act = outs[0][..., off:]
            ref = N.stemskip_node(a["y"], pre.weight, pre.bias, pre.eps, arg=arg, act_stored=act, dpool=go[1], dskip=go[0][..., off:])
            near(act, ref.act, f"{node.name} skip")
            near(outs[1], ref.pool, f"{node.name} pool")                 # on float64's own maxima
            near(outs[1], ref.pool_at_arg, f"{node.name} pool at arg")   # the device's choice is a maximum, to rounding
            # the pool is the maximum of the STORED skip values, bit for bit
            same(outs[1], F.max_pool2d(act.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(act.dtype).contiguous(),
                 f"{node.name} pool of the stored skip")
            near(grads["y"], ref.dy, f"{node.name} dy")
            norm_checks(node, pre, bn, ref, 3e-3)
            bn.eval()
            with torch.no_grad():
                be, pe = U.stem_tail_skip(a["y"], None, bn, off)
            re_ = N.stemskip_node(a["y"], bn.weight, bn.bias, bn.eps, running=(bn.running_mean, bn.running_var))
            near(be[..., off:], re_.act, f"{node.name} eval skip")
            near(pe, re_.pool, f"{node.name} eval pool")
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
                # B = 2: the branch's gradients are eps-driven (tests/test_deeplabv3_nodes_gpu.py's docstring) -- their errors bounded
                # relative to the size the same gradients would have without the batch norm's cancellation, |gamma| rstd |dpooled|
                # carried through the 1x1 weight (dx: and the 1 / HW broadcast, H W of this stride-16 map) or against the sample means (dw)
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
        elif node.kind == "dw":
            R = len(o["rates"])
            ref = N.dw_node(a["x"], [a[f"w{r}"] for r in range(R)], o["rates"], dys=go)
            for r in range(R):
                near(outs[r], ref.ys[r], f"{node.name} y{r} (rate {o['rates'][r]})")
                bar(rel(grads[f"w{r}"], ref.dws[r]), 5e-4, f"{node.name} dw{r} (rate {o['rates'][r]})", "depthwise dw")
            near(grads["x"], ref.dx, f"{node.name} dx")
        elif node.kind == "upcat":
            Ca, Cs, s = a["a"].shape[-1], a["skip"].shape[-1], o["scale"]
            out64, da64, _ = N.upcat_node(a["a"], a["skip"], s, o["ld"], dout=go[0])
            near(outs[0][..., :Ca], out64[..., :Ca], f"{node.name} up-sampled channels")
            same(outs[0][..., Ca: Ca + Cs], a["skip"], f"{node.name} skip channels")
            assert not outs[0][..., Ca + Cs:].any(), f"{node.name}: the pad channels"
            near(grads["a"], da64, f"{node.name} da")
            same(grads["skip"], go[0][..., Ca: Ca + Cs], f"{node.name} dskip")
            # one statement of the arithmetic: the stand-alone up-sampling and its adjoint, bit for bit
            a2 = _fresh(a["a"])
            up = D.upsample_bilinear_ac(a2, s)
            same(outs[0][..., :Ca], up.detach(), f"{node.name} = upsample_bilinear_ac")
            up.backward(go[0][..., :Ca].contiguous())
            same(grads["a"], a2.grad, f"{node.name} da = upsample_bilinear_ac's")
        elif node.kind in ("up2cat", "up2into"):
            Cx = a["x"].shape[-1]
            skip = a["skip"] if node.kind == "up2cat" else a["buf"][..., Cx:]      # (up2into: what the stem wrote beside)
            out64, _, _ = N.up2cat_node(a["x"], skip, dout=go[0])
            assert torch.equal(outs[0].double(), out64), f"{node.name}: moved values"
            sum_of_four(grads["x"], go[0], Cx, f"{node.name} dx")
            if node.kind == "up2into":
                same(grads["buf"], go[0], f"{node.name}: the gradient handed on to the buffer's producer")
            elif skip is not None:
                same(grads["skip"], go[0][..., Cx:], f"{node.name} dskip")
        else:
            up64, dx64 = N.upsample_node(a["x"], o["scale"], dout=go[0])
            near(outs[0], up64, f"{node.name} up")
            near(grads["x"], dx64, f"{node.name} dx")
    print(f"\n{run.case}: worst value / bar:", ", ".join(f"{k} {v:.1e} / {lim:.0e}" for k, (v, lim) in sorted(worst.items())))
    return worst


# ------------------------------------------------------------------------------------------------ wiring
def check_edges(run, diff_inputs):
    """every node input except the network's own traces to a recorded output; a single-consumer edge is bit-identical, a
    multi-consumer one within (k - 1) 2^-8 sum|terms| of the float64 sum; the identity edges of the residual blocks; conv1's dx is the
    network's input gradient.  Returns {producer name: sorted consumers} of the multi-consumer tensors for the caller's literal
    assertion."""
    rec, m = run.rec, run.model
    nodes = rec.nodes
    consumers, unmatched = {}, []
    for node in nodes:
        for slot in diff_inputs[node.kind]:
            if node.args.get(slot) is None:
                continue
            if slot in node.src:
                consumers.setdefault(node.src[slot], []).append((node, slot))
            else:
                unmatched.append(f"{node.name} {slot}")
    # a model change that puts a copy between two nodes must fail here, not drop the edge from the checks below
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
    # the identity edges: each residual batch norm's res is conv1's passthrough output (no downsample) or the downsample's norm
    for node in nodes:
        if node.kind == "bn" and node.args["res"] is not None:
            j, o = node.src["res"]
            blk = node.name.rsplit(".", 1)[0]
            assert (nodes[j].name, o) in ((f"{blk}.conv1", 2), (f"{blk}.downsample.1", 0)), (node.name, nodes[j].name, o)
    same(rec["encoder.conv1"].grad("x")[..., :m.in_channels].float(), run.dx, "encoder.conv1 dx (the network's input gradient)")
    return multi


def check_head_gradient(run, node):
    """the network's last node receives dy cast to bf16, and zeros in the output channels the head was padded by"""
    cout = run.model.out_channels
    same(node.gout[0][..., :cout], run.dy.to(torch.bfloat16), f"{node.name} dy")
    assert not node.gout[0][..., cout:].any(), f"{node.name} dy: the padded output channels"


def last_blocks(m):
    return {li: f"encoder.layer{li}.{len(getattr(m.encoder, f'layer{li}')) - 1}.bn2" for li in (1, 2, 3, 4)}


def check_parameter_gradients_are_the_node_replays(run):
    m = run.model
    names = {id(p): n for n, p in m.named_parameters()}
    owner = {}
    for node, (_, grads, _, _) in zip(run.rec.nodes, replays(run)):
        for slot, p in node.params().items():
            assert id(p) not in owner, f"{node.name} {slot}: parameter already taken by {owner[id(p)]}"
            owner[id(p)] = f"{node.name} {slot}"
            same(run.g_none[names[id(p)]], to_param(grads[slot], p).to(p.dtype), f"{node.name} {slot}: p.grad")
    for name, p in m.named_parameters():
        assert id(p) in owner, f"{name}: no node owns it"


# ------------------------------------------------------------------------------------------------ sink route
def check_sink_route_adds_into_grad(run):
    """p.grad pre-filled, and under FlatDDP (every .grad a view of one non-zero flat buffer, as bench.py builds it): p.grad = prefill +
    the gradient of the .grad-is-None run, bit for bit (same generator state: the same Dropout draw)"""
    from py4cast_amd.trainer import FlatDDP

    m = run.model
    g = torch.Generator(device=run.x.device).manual_seed(11)
    prefill = {n: (torch.rand(p.shape, device=p.device, generator=g) + 0.5) * (1 - 2 * (torch.rand(p.shape, device=p.device, generator=g) < 0.5))
               for n, p in m.named_parameters()}
    for n, p in m.named_parameters():
        p.grad = prefill[n].clone()
    run.step(m, run.x, run.dy)
    if run.mask is not None:
        same(m.last_dropout_mask, run.mask, "the Dropout draw of the rerun")
    for n, p in m.named_parameters():
        same(p.grad, prefill[n] + run.g_none[n], f"prefilled .grad: {n}")
    ddp = FlatDDP(m, 1)
    for n, p in m.named_parameters():
        assert p.grad.data_ptr() >= ddp.flat_grad.data_ptr(), n
        p.grad.copy_(prefill[n])
    run.step(m, run.x, run.dy)
    for n, p in m.named_parameters():
        same(p.grad, prefill[n] + run.g_none[n], f"FlatDDP .grad: {n}")
