"""
The float64 node references of tests/halfunet_nodes.py prove themselves, without a device: chained from random inputs and weights --
forward, then backward in the plan's order with the plan's intermediate buffers and the references' own decisions -- they give every
node value and every parameter / input gradient of oracle.halfunet.HalfUNetRef(...).double() under autograd to 1e-10 (a margin over
double rounding; measured <= 2e-14), for BatchNorm in training and eval mode and for GroupNorm, on a 48 x 80 grid (H != W, coarsest
level 3 x 5).  And the library's layout query: offsets ascending, regions disjoint, inside the sizes p4c_halfunet_workspace_bytes reports.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import halfunet_nodes as N  # noqa: E402

B, H, W, CIN, COUT = 2, 48, 80, 5, 3
TIGHT = 1e-10
NFK = 4   # channels of the stand-alone up-sampling checks


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous()


def _net(norm, seed):
    from oracle.halfunet import HalfUNetRef

    torch.manual_seed(seed)
    net = HalfUNetRef(CIN, COUT, norm=norm, groups=8).double()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.GroupNorm)):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return net


def _blocks(net):
    """[(conv, norm, relu)] of the 12 blocks in plan order"""
    out = []
    for name, attr in zip(("enc1", "enc2", "enc3", "enc4", "enc5", "decoder"), ("encoder1", "encoder2", "encoder3", "encoder4", "encoder5", "decoder")):
        seq = getattr(net, attr)
        for j in (1, 2):
            out.append((getattr(seq, f"{name}conv{j}"), getattr(seq, f"{name}norm{j}"), getattr(seq, f"{name}relu{j}")))
    return out


def _params(net):
    ps = []
    for c, n, _ in _blocks(net):
        ps += [c.weight, n.weight, n.bias]
    return ps + [net.outconv.weight]


def _autograd_run(net, x, dy):
    """forward + backward of the torch network with every node tensor captured and its gradient retained"""
    cap = {"Y": [], "A": [], "P": [], "S": None}
    hooks = []

    def keep(store):
        def hook(_m, _inp, out):
            out.retain_grad()
            store.append(out)
        return hook

    for c, _n, r in _blocks(net):
        hooks.append(c.register_forward_hook(keep(cap["Y"])))
        hooks.append(r.register_forward_hook(keep(cap["A"])))
    for p in (net.pool1, net.pool2, net.pool3, net.pool4):
        hooks.append(p.register_forward_hook(keep(cap["P"])))

    def dec_in(_m, inp):
        inp[0].retain_grad()
        cap["S"] = inp[0]
    hooks.append(net.decoder[0].register_forward_pre_hook(dec_in))
    xg = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = net(xg)
    y.backward(dy.permute(0, 3, 1, 2).contiguous())
    for h in hooks:
        h.remove()
    return cap, y, xg.grad


@pytest.mark.parametrize("norm,training", [("batch", True), ("batch", False), ("group", True)])
def test_chained_references_match_the_torch_network_under_autograd(norm, training):
    net = _net(norm, seed=11)
    net.train(training)
    spec = N.Spec(bf16=False, norm=norm, groups=8, eps=1e-5, momentum=0.1, training=training)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, W, CIN, generator=g, dtype=torch.float64)
    dy = torch.randn(B, H, W, COUT, generator=g, dtype=torch.float64)
    blocks = _blocks(net)
    running = [(n.running_mean.clone(), n.running_var.clone()) for _c, n, _r in blocks] if norm == "batch" else None
    params = [p.detach().clone() for p in _params(net)]

    cap, y, dx = _autograd_run(net, x, dy)
    fw = N.chain_forward(x, params, spec, running)
    bw = N.chain_backward(fw, params, spec, dy, CIN)

    # the inputs decide nothing by a hair: no 2x2 window ties, no pre-activation within 1e-9 of zero (level 0 .. 3 are pooled)
    for i in range(N.NCONV):
        z = N.preact(fw.Y[i], fw.norm[i][0], fw.norm[i][1])
        assert float(z.abs().min()) > 1e-9, f"block {i}: a pre-activation within 1e-9 of zero"
    for k in range(N.NLEV - 1):
        win = N._windows(fw.A[2 * k + 1])
        top = win.topk(2, -1).values
        tie = (top[..., 0] == top[..., 1]) & (top[..., 0] > 0)   # (windows that are zero throughout route to the first element: both)
        assert not bool(tie.any()), f"level {k}: a 2x2 window with two equal positive maxima"

    worst = {}

    def check(what, got, ref):
        e = rel(got, ref)
        worst[what.split()[0]] = max(worst.get(what.split()[0], 0.0), e)
        assert e < TIGHT, f"{norm} training={training}: {what}: {e:.3e}"

    for i in range(N.NCONV):
        check(f"Y block {i}", fw.Y[i], nhwc(cap["Y"][i]))
        check(f"A block {i}", fw.A[i], nhwc(cap["A"][i]))
        check(f"dY block {i}", bw.dY[i], nhwc(cap["Y"][i].grad))
        check(f"dA block {i}", bw.dA[i], nhwc(cap["A"][i].grad))
        conv, nm, _ = blocks[i]
        check(f"dW block {i}", bw.dW[i], conv.weight.grad)
        check(f"dgamma block {i}", bw.dgamma[i], nm.weight.grad)
        check(f"dbeta block {i}", bw.dbeta[i], nm.bias.grad)
        if norm == "batch" and training:
            rm, rv = N.running_update(running[i][0], running[i][1], fw.stats[i][0], fw.stats[i][2], spec.momentum)
            check(f"running_mean block {i}", rm, nm.running_mean)
            check(f"running_var block {i}", rv, nm.running_var)
            assert all(bool((a == a[0]).all()) for a in fw.norm[i]), f"block {i}: BatchNorm rows differ between samples"
        if norm == "batch" and not training:
            assert float(bw.k1[i].abs().max()) == 0.0 and float(bw.k2[i].abs().max()) == 0.0
            check(f"eval-dY block {i}", bw.dY[i], N._bc(fw.norm[i][0]) * bw.dA[i] * (N.preact(fw.Y[i], fw.norm[i][0], fw.norm[i][1]) > 0))
    for k in range(1, N.NLEV):
        check(f"P level {k}", fw.P[k], nhwc(cap["P"][k - 1]))
        # x pass then y pass is the adjoint of torch's up-sampling
        up = torch.nn.Upsample(scale_factor=1 << k, mode="bilinear", align_corners=False)
        a = torch.randn(B, NFK, H >> k, W >> k, generator=g, dtype=torch.float64).requires_grad_(True)
        gs = torch.randn(B, H, W, NFK, generator=g, dtype=torch.float64)
        up(a).backward(gs.permute(0, 3, 1, 2))
        check(f"up-adjoint level {k}", N.up_adj_y(N.up_adj_x(gs, 1 << k), 1 << k), nhwc(a.grad))
        check(f"upsample level {k}", N.upsample(nhwc(a), 1 << k), nhwc(up(a)))
    check("S", fw.S, nhwc(cap["S"]))
    check("dS", bw.G0, nhwc(cap["S"].grad))
    check("y", fw.y, nhwc(y))
    check("dWout", bw.dWout, net.outconv.weight.grad)
    check("dx", bw.dx, nhwc(dx))
    print(f"{norm} training={training}: worst relative error per quantity:", {k: f"{v:.1e}" for k, v in worst.items()})


def test_first_maximum_rule_and_tie_routing():
    """the pool adjoint sends a window's gradient to the FIRST maximum in row-major order -- also where all four are equal (a window of
    zeros after the ReLU)"""
    a = torch.tensor([[1.0, 3.0, 0.0, 0.0], [3.0, 2.0, 0.0, 0.0]], dtype=torch.float64).view(1, 2, 4, 1)
    dP = torch.tensor([5.0, 7.0], dtype=torch.float64).view(1, 1, 2, 1)
    want = torch.tensor([[0.0, 5.0, 7.0, 0.0], [0.0, 0.0, 0.0, 0.0]], dtype=torch.float64).view(1, 2, 4, 1)
    assert torch.equal(N.pool_route(a, dP), want)
    assert N.pool_margin(a) == 0.0


def _regions(lay, B, H, W):
    n = [B * (H >> k) * (W >> k) * 64 * lay["elem_bytes"] for k in range(5)]
    saved = [(f"Y[{i}]", lay["Y"][i], n[N.LEVEL[i]]) for i in range(12)] + [(f"P[{k}]", lay["P"][k], n[k]) for k in range(1, 5)] + \
            [("S", lay["S"], n[0])] + [(f"norm[{i}]", lay["norm"][i], 4 * B * 64 * 4) for i in range(12)]
    scratch = []
    for s in (0, 1):
        for i in range(12):
            scratch += [(f"k1[{s}][{i}]", lay["k1"][s][i], B * 64 * 4), (f"k2[{s}][{i}]", lay["k2"][s][i], B * 64 * 4)]
    scratch += [("G0", lay["G0"], n[0]), ("TB", lay["TB"], n[0] // 2 + n[0] // 4 + n[0] // 8 + n[0] // 16)]
    for s in (0, 1):
        scratch += [(f"DY[{s}][{i}]", lay["DY"][s][i], n[N.LEVEL[i]]) for i in range(12)]
    return saved, scratch


# B, H, W, cin, cout, dx_channels, storage, compute, norm: the shapes of tests/test_halfunet_nodes_gpu.py and the benchmark's
LAYOUT_CASES = [(2, 64, 64, 69, 60, 64, "bf16", "bf16", 0), (2, 256, 96, 69, 60, 64, "bf16", "bf16", 0), (3, 48, 80, 46, 21, 46, "bf16", "bf16", 1),
                (33, 16, 48, 69, 60, 64, "bf16", "bf16", 0), (2, 32, 64, 138, 60, 120, "bf16", "bf16", 0), (2, 32, 64, 46, 21, 46, "f32", "bf16", 0),
                (2, 32, 48, 10, 1, 10, "f32", "f32", 0), (2, 512, 512, 69, 60, 60, "bf16", "bf16", 0)]


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_layout_query(case):
    """p4c_halfunet_layout needs no device: every region it names starts where or after the one before it ends, ends inside its
    workspace, and the parameter offsets are those of the model's flat parameter vector"""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops_model as om
    from py4cast_amd._lib_model import HalfUNetDesc
    from py4cast_amd.halfunet import pad32

    B_, H_, W_, cin, cout, dxc, storage, compute, norm = case
    code = {"f32": L.F32, "bf16": L.BF16}
    desc = HalfUNetDesc(B_, H_, W_, cin, pad32(cin), cout, dxc, code[storage], norm, 8, 0, 1e-5, 0.1, code[compute], 0)
    lay = om.halfunet_layout(desc)
    sb, cb = ctypes.c_size_t(), ctypes.c_size_t()
    L.call("p4c_halfunet_workspace_bytes", ctypes.byref(desc), ctypes.byref(sb), ctypes.byref(cb))
    assert lay["saved_bytes"] == sb.value and lay["scratch_bytes"] == cb.value
    assert lay["elem_bytes"] == (2 if storage == "bf16" else 4) and lay["P"][0] == -1
    for regions, size in zip(_regions(lay, B_, H_, W_), (sb.value, cb.value)):
        end, prev = 0, "the start"
        for name, off, nbytes in regions:
            assert off >= end, f"{name} at {off} begins before {prev} ends ({end})"
            assert off % 4 == 0
            end, prev = off + nbytes, name
        assert end <= size, f"{prev} ends at {end}, beyond the workspace ({size})"
    # parameters: conv weight, gamma, beta per block, then the output convolution, back to back
    off = 0
    for i in range(12):
        assert (lay["w"][i], lay["gamma"][i], lay["beta"][i]) == (off, off + 4 * 64 * (cin if i == 0 else 64) * 9, off + 4 * 64 * (cin if i == 0 else 64) * 9 + 256)
        off = lay["beta"][i] + 256
    assert lay["wout"] == off and lay["params_bytes"] == off + 4 * cout * 64
    assert lay["params_bytes"] == 4 * L.lib().p4c_halfunet_param_count(ctypes.byref(desc))
    with pytest.raises(L.P4CError):
        om.halfunet_layout(HalfUNetDesc(B_, H_ + 1, W_, cin, pad32(cin), cout, dxc, code[storage], norm, 8, 0, 1e-5, 0.1, code[compute], 0))
