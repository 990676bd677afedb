"""
UNet (py4cast_amd/unet.py) node by node: one forward / backward of UNetMI355X under tests/unet_nodes.py's recorder, then for every
recorded node (the 3x3 / 1x1 convolutions, the batch norms, the encoder tails, the transposed convolutions):

* replay: the node alone on its recorded inputs and incoming gradient, with fresh parameter leaves, gives the in-network forward
  output and input / weight / bias gradients BIT FOR BIT (every native reduction has a fixed order);
* float64: the replay against the float64 node reference -- forward outputs against the reference's own ReLU (an output wrongly left
  at zero shows), gradients with every decision (ReLU mask, pool routing) taken from the device's stored values -- so no gradient
  comparison crosses a decision and the bars are the kernel tests' (tests/test_gemm_gpu.py, tests/test_unet_gpu.py):
  bf16 maps <= 6e-3 of the largest magnitude per element and <= 3e-3 in the 2-norm, convolution / transposed-convolution weight and
  bias gradients <= 5e-4, batch-norm gamma / beta gradients <= 5e-3 (3e-3 for the encoder tail), running mean / var <= 1e-4 with
  num_batches_tracked advanced by exactly one; fp32 nodes <= 1e-5 on outputs and <= 1e-4 on gradients; plus an eval-mode forward of
  every batch norm on the running statistics the training call left;
* wiring: the gradient each node's output received is, bit for bit, the input gradient its consumer produced (at the concatenation
  buffer: the decoder's first convolution's channels [:C] reach the transposed convolution, [C:] the encoder tail's skip), and the
  network's p.grad is the node replays' parameter gradient -- every parameter belongs to exactly one node;
* sink route (bf16): the same backward with every .grad pre-filled, and under FlatDDP (every .grad a view of one flat buffer, as
  bench.py builds it): p.grad = prefill + the gradient of the first run, bit for bit (the reductions add their finished fp32 sum once).

fp32 (the parity flavour) records the native nodes only -- the batch norms and encoder tails; its convolutions are the library's.

Measured at the benchmark size (2 x 512 x 512, F = 60, f = 64; worst node / bar): bf16 maps 5.8e-3 / 6e-3 per element and 2.3e-3 / 3e-3
in the 2-norm (bf16 rounding of the stored maps), convolution / transposed-convolution weight and bias gradients 2.6e-6 / 5e-4, BN
gamma / beta gradients 2.6e-7 / 5e-3, encoder tail 2.9e-7 / 3e-3, running mean / var 4.6e-8 / 1e-4; fp32: outputs 9.7e-8 / 1e-5,
gradients 3.8e-7 / 1e-4.  The whole file takes about 13 s on one MI355X.
"""
import copy
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import unet_nodes as N  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (B, H, W, in_channels, out_channels, init_features, flavour)
CASES = {
    "toy-f16-bf16": (2, 64, 64, 69, 60, 16, "bf16"),
    "toy-f64-bf16": (2, 64, 64, 69, 60, 64, "bf16"),
    "toy-f16-f32": (2, 64, 64, 69, 60, 16, "f32"),
    "toy-f64-f32": (2, 64, 64, 69, 60, 64, "f32"),
    "bench-bf16": (2, 512, 512, 69, 60, 64, "bf16"),      # bench.py --model UNet: 2 x 512 x 512, F = 60 (69 input channels -> 72)
    "bench-f32": (2, 512, 512, 69, 60, 64, "f32"),
    "titan-bf16": (2, 512, 640, 46, 21, 64, "bf16"),      # the Titan grid; 46 input channels -> 48
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


def to_param(g, p):
    """a node's gradient of the (padded) operand it was given, as the parameter's own shape (encoder1's zero input columns, the head's
    zero output rows sliced off)"""
    return g[tuple(slice(0, s) for s in p.shape)]


def make_model(case, dev):
    from py4cast_amd.unet import UNetMI355X, UNetSettings

    B, H, W, cin, cout, f, key = CASES[case]
    torch.manual_seed(0)
    m = UNetMI355X(cin, cout, (H, W), UNetSettings(init_features=f, compute_dtype=key, activation_dtype=key)).to(dev).train()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.3, 0.3)
            elif getattr(mod, "bias", None) is not None:
                mod.bias.uniform_(-0.3, 0.3)
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(B, H, W, cin, device=dev, generator=g)
    dy = torch.randn(B, H, W, cout, device=dev, generator=g)
    return m, x, dy


def step(m, x, dy):
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
    yield SimpleNamespace(case=request.param, model=m, x=x, dy=dy, y=y, dx=dx, rec=rec, g_none=g_none, native=m.native)
    del m, rec, g_none
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ replay
def replay(node):
    """the node alone on its recorded inputs, its recorded incoming gradient and fresh parameter leaves: (outputs, {slot: gradient},
    the node's batch norm after the call or None)"""
    from py4cast_amd import ops_gemm as G
    from py4cast_amd import unet as U

    a = node.args

    def leaf(t):
        return None if t is None else t.clone().requires_grad_(True)

    bn = None
    if node.kind == "conv":
        x, w, b = leaf(a["x"]), leaf(a["w"]), leaf(a["b"])
        out = G.conv2d_nhwc(x, w, b, want_stats=node.opts["want_stats"])
        outs = list(out) if node.opts["want_stats"] else [out, None]
        outs[0].backward(node.gout[0].clone())
        grads = {"x": x.grad, "w": w.grad, "b": None if b is None else b.grad}
    elif node.kind == "bn":
        bn = copy.deepcopy(node.pre)
        y = leaf(a["y"])
        outs = [G.batch_norm_act(y, None if a["stats"] is None else a["stats"].clone(), bn, slope=node.opts["slope"])]
        outs[0].backward(node.gout[0].clone())
        grads = {"y": y.grad, "gamma": bn.weight.grad, "beta": bn.bias.grad}
    elif node.kind == "tail":
        bn = copy.deepcopy(node.pre)
        y = leaf(a["y"])
        outs = list(U.enc_tail(y, None if a["stats"] is None else a["stats"].clone(), bn))
        pairs = [(o, g.clone()) for o, g in zip(outs, node.gout) if g is not None]
        torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs])
        grads = {"y": y.grad, "gamma": bn.weight.grad, "beta": bn.bias.grad}
    else:
        x, w, b = leaf(a["x"]), leaf(a["w"]), leaf(a["b"])
        base = a["buf"].clone().requires_grad_(True)
        outs = [U.upconv_into(x, w, b, base.clone(), grad_owned=node.opts["grad_owned"])]
        outs[0].backward(node.gout[0].clone())        # (grad_owned: the backward zeroes its incoming gradient in place)
        grads = {"x": x.grad, "w": w.grad, "b": None if b is None else b.grad, "buf": base.grad}
    torch.cuda.synchronize()
    return [None if o is None else o.detach() for o in outs], grads, bn


def test_replay_is_bit_identical(run):
    for node in run.rec.nodes:
        outs, grads, bn = replay(node)
        for j, (o, want) in enumerate(zip(outs, node.out)):
            if want is None:
                continue
            if node.kind == "tail" and j == 0:         # the buffer's first half is the transposed convolution's, uninitialised here
                C = node.args["y"].shape[-1]
                o, want = o[..., C:], want[..., C:]
            same(o, want, f"{node.name} out{j}")
        for slot, g in grads.items():
            want = node.grad(slot)
            if want is None and g is None:
                continue
            same(g, want, f"{node.name} d{slot}")
        if bn is not None:
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                same(getattr(bn, k), getattr(node.post, k), f"{node.name} {k}")


# ------------------------------------------------------------------------------------------------ float64
def test_nodes_against_float64(run):
    """every node's replay against its float64 reference (decisions from the stored values); prints the worst value met per bar"""
    native = run.native
    worst = {}

    def bar(v, limit, what, key):
        worst[key] = max(worst.get(key, (0.0, limit)), (v, limit))
        assert v <= limit, f"{what}: {v:.2e} > {limit:.0e}"

    def near(got, ref, what, fp32_bar):
        if native:
            got, ref = got.detach().double(), ref.detach().double()
            assert got.shape == ref.shape, (what, got.shape, ref.shape)
            bar(float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)), 6e-3, f"{what} (max)", "bf16 map, max")
            bar(rel(got, ref), 3e-3, f"{what} (2-norm)", "bf16 map, 2-norm")
        else:
            bar(rel(got, ref), fp32_bar, what, "fp32 out" if fp32_bar == 1e-5 else "fp32 grad")

    for node in run.rec.nodes:
        outs, grads, bn = replay(node)
        a = node.args
        if node.kind == "conv":
            y64, dx64, dw64, db64 = N.conv_node(a["x"], a["w"], a["b"], dy=node.gout[0])
            near(outs[0], y64, f"{node.name} y", None)
            near(grads["x"], dx64, f"{node.name} dx", None)
            bar(rel(grads["w"], dw64), 5e-4, f"{node.name} dw", "conv / upconv dw, db")
            if db64 is not None:
                bar(rel(grads["b"], db64), 5e-4, f"{node.name} db", "conv / upconv dw, db")
        elif node.kind == "up":
            C = a["w"].shape[1]
            up64, dx64, dw64, db64 = N.upconv_node(a["x"], a["w"], a["b"], dup=node.gout[0][..., :C])
            near(outs[0][..., :C], up64, f"{node.name} up", None)
            same(outs[0][..., C:], a["buf"][..., C:], f"{node.name} skip half")
            near(grads["x"], dx64, f"{node.name} dx", None)
            bar(rel(grads["w"], dw64), 5e-4, f"{node.name} dw", "conv / upconv dw, db")
            bar(rel(grads["b"], db64), 5e-4, f"{node.name} db", "conv / upconv dw, db")
            same(grads["buf"][..., C:], node.gout[0][..., C:], f"{node.name} dbuf[..., C:]")
            assert not grads["buf"][..., :C].any(), f"{node.name} dbuf[..., :C] is not zero"
        else:
            pre = node.pre
            if node.kind == "bn":
                ref = N.bn_node(a["y"], pre.weight, pre.bias, pre.eps, mask=outs[0] > 0, dout=node.gout[0])
                own = N.bn_node(a["y"], pre.weight, pre.bias, pre.eps)
                out, gbar = outs[0], 5e-3
            else:
                C = a["y"].shape[-1]
                act = outs[0][..., C:]
                ref = N.tail_node(a["y"], pre.weight, pre.bias, pre.eps, act=act, dskip=node.gout[0][..., C:], dpool=node.gout[1])
                own = N.tail_node(a["y"], pre.weight, pre.bias, pre.eps)
                same(outs[1], N.max_pool(act), f"{node.name} pool")          # the max of the stored activations, exactly
                out, gbar = act, 3e-3
            # the forward against float64's OWN ReLU: an output wrongly left at zero must show (a decision flipped at |z| ~ rounding
            # moves the value by about the rounding); the backward against the reference that takes the stored output's decisions
            near(out, own.out, f"{node.name} out", 1e-5)
            near(grads["y"], ref.dy, f"{node.name} dy", 1e-4)
            for slot, r64 in (("gamma", ref.dgamma), ("beta", ref.dbeta)):
                bar(rel(grads[slot], r64), gbar if native else 1e-4, f"{node.name} d{slot}", f"{node.kind} dgamma, dbeta")
            rm, rv = N.running_update(pre, ref, pre.momentum)
            bar(rel(bn.running_mean, rm), 1e-4, f"{node.name} running_mean", "running mean, var")
            bar(rel(bn.running_var, rv), 1e-4, f"{node.name} running_var", "running mean, var")
            assert int(bn.num_batches_tracked) == int(pre.num_batches_tracked) + 1, f"{node.name} num_batches_tracked"
            # eval mode on the running statistics this call left
            bn.eval()
            running = (bn.running_mean, bn.running_var)
            if node.kind == "bn":
                from py4cast_amd import ops_gemm as G

                with torch.no_grad():
                    oe = G.batch_norm_act(a["y"], None, bn, slope=node.opts["slope"])
                re_ = N.bn_node(a["y"], bn.weight, bn.bias, bn.eps, running=running)
            else:
                from py4cast_amd import unet as U

                with torch.no_grad():
                    be, pe = U.enc_tail(a["y"], None, bn)
                oe = be[..., C:]
                re_ = N.tail_node(a["y"], bn.weight, bn.bias, bn.eps, running=running)
                same(pe, N.max_pool(oe), f"{node.name} eval pool")
            near(oe, re_.out, f"{node.name} eval out", 1e-5)
        del outs, grads
    print(f"\n{run.case}: worst value / bar:", ", ".join(f"{k} {v:.1e} / {lim:.0e}" for k, (v, lim) in sorted(worst.items())))


# ------------------------------------------------------------------------------------------------ wiring
DIFF_INPUTS = {"conv": ("x",), "bn": ("y",), "tail": ("y",), "up": ("x", "buf")}


def test_wiring_is_bit_identical(run):
    rec, m = run.rec, run.model
    nodes = rec.nodes
    # every recorded input that is a recorded output: its consumer's input gradient is what the producer's output received
    unmatched = []
    for node in nodes:
        for slot in DIFF_INPUTS[node.kind]:
            if slot in node.src:
                j, o = node.src[slot]
                same(nodes[j].gout[o], node.grad(slot), f"{node.name} d{slot} -> {nodes[j].name} out{o}")
            else:
                unmatched.append(f"{node.name} {slot}")
    if run.native:
        # on the bf16 route every node input but the network's own is a recorded output (44 edges): a model change that puts a copy
        # between two nodes must fail here, not drop the edge from the check above
        assert unmatched == ["enc1.conv1 x"], f"node inputs not traced to a recorded output: {unmatched}"
        for lvl in (1, 2, 3, 4):
            up, c1, tail = rec[f"upconv{lvl}"], rec[f"dec{lvl}.conv1"], rec[f"enc{lvl}.norm2"]
            C = up.args["w"].shape[1]
            assert c1.src["x"] == (nodes.index(up), 0) and up.src["buf"] == (nodes.index(tail), 0), f"dec{lvl}: concatenation buffer"
            dxc = c1.grad("x")
            same(dxc[..., :C], up.gout[0][..., :C], f"dec{lvl}.conv1 dx[:, :C]")
            same(dxc[..., C:], tail.gout[0][..., C:], f"dec{lvl}.conv1 dx[:, C:] (enc{lvl} skip)")
            nxt = rec[f"enc{lvl + 1}.conv1"] if lvl < 4 else rec["bottleneck.conv1"]
            same(tail.gout[1], nxt.grad("x"), f"enc{lvl} dpool")
        head = rec["head"]
        cout = m.out_channels
        same(head.gout[0][..., :cout], run.dy.to(torch.bfloat16), "head dy")
        assert not head.gout[0][..., cout:].any(), "head dy: the padded output rows"
        same(rec["enc1.conv1"].grad("x")[..., :m.in_channels].float(), run.dx, "enc1.conv1 dx (the network's input gradient)")
    # the network's p.grad is the sum of the node replays' parameter gradients; each parameter belongs to exactly one node
    owner = {}
    for node in nodes:
        _, grads, _ = replay(node)
        for slot, p in node.params().items():
            assert id(p) not in owner, f"{node.name} {slot}: parameter already taken by {owner[id(p)]}"
            owner[id(p)] = node.name
            same(run.g_none[_name(m, p)], to_param(grads[slot], p).to(p.dtype), f"{node.name} {slot}: p.grad")
    for name, p in m.named_parameters():
        if run.native or isinstance(_module_of(m, name), torch.nn.BatchNorm2d):
            assert id(p) in owner, f"{name}: no node owns it"


def _name(m, p):
    for n, q in m.named_parameters():
        if q is p:
            return n
    raise KeyError


def _module_of(m, name):
    return m.get_submodule(name.rsplit(".", 1)[0])


# ------------------------------------------------------------------------------------------------ sink route
def test_sink_route_adds_into_grad(run):
    """bf16 route: p.grad pre-filled (conv2d_nhwc / upconv_into then add their weight gradients into it in place, through GradQueue's deferred
    flush; encoder1's padded weight, the head and the batch norms go through autograd's accumulation), and under FlatDDP with a
    non-zero flat buffer: p.grad = prefill + the gradient of the .grad-is-None run, bit for bit.  The fp32 flavour has no sink route
    (its convolutions are the library's, every parameter gradient goes through autograd): nothing to check there."""
    from py4cast_amd.trainer import FlatDDP

    if not run.native:
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
