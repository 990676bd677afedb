"""HalfUNet's module path (the HalfUNetSettings combinations the fused plan is not built for), everything of
tests/test_halfunet_settings_bf16_gpu.py that needs no device: the seeds, shapes and state-dict plumbing against the float64 oracle in
fp32, the float64 node references of tests/halfunet_module_nodes.py against torch.autograd on plain nn.Conv2d modules, the condition of
the device test (no dead node, the route facts) on the recorder with stand-in nodes, and the sensitivity of the comparison."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import halfunet_module_nodes as N

# (CI, CO, ks, groups): the convolutions of the six settings rows -- 21 -> 32, 32 -> 32, 32 -> 12 (1x1), 48 -> 24, 64 -> 32, 64 -> 64,
# and the depthwise 32 of the Ghost module's cheap operation
CHANNELS = [(21, 32, 3, 1), (32, 32, 3, 1), (32, 12, 1, 1), (48, 24, 3, 1), (64, 32, 3, 1), (64, 64, 3, 1), (32, 32, 3, 32)]


@pytest.mark.parametrize("row,H,W", N.CASES, ids=N.CASE_IDS)
def test_module_path_agrees_with_the_oracle_in_fp32(row, H, W):
    """`_forward_modules` on the CPU in fp32 (the library branches) against HalfUNetRef(...).double() on one state dict: output <= 1e-4,
    input gradient and every parameter gradient <= 5e-3, running statistics <= 1e-4 -- the bars of
    test_halfunet_yaml_settings_match_oracle, at every settings row and grid of the device test, with its seeds.  The oracle run in
    fp32 must be within the same bars of its float64 run: a case where it is not (a badly conditioned draw) could not carry them."""
    model, ref = N.make_models(row, H, W, bf16=False)
    x, gy = N.make_inputs(H, W)
    got = N.train_then_eval(model, x, gy, "cpu", forward=model._forward_modules)
    want = N.oracle_train_then_eval(ref, x, gy)
    # the case is conditioned well enough for the bars to mean something: the oracle itself in fp32 is within them of its float64 run
    own = N.oracle_train_then_eval(ref, x, gy, dtype=torch.float32)
    assert N.rel(own["output"], want["output"]) < 1e-4
    assert max(N.rel(own[k], want[k]) for k in ("input gradient", "parameter gradients")) < 5e-3
    assert got["output"].shape == (N.B, H, W, N.COUT)
    assert N.rel(got["output"], want["output"]) < 1e-4
    assert N.rel(got["eval output"], want["eval output"]) < 1e-4
    assert N.rel(got["input gradient"], want["input gradient"]) < 5e-3
    assert set(got["named"]) == set(want["named"])
    for n, g in got["named"].items():
        r = want["named"][n]
        scale = float(r.norm())
        if n.endswith(".bias") and n[:-4] + "weight" in want["named"]:
            scale = max(scale, 1e-2 * float(want["named"][n[:-4] + "weight"].norm()))
        assert float((g - r).norm()) < 5e-3 * scale, (n, float((g - r).norm()), scale)
    if ROW_HAS_STATS(row):
        assert N.rel(got["running statistics"], want["running statistics"]) < 1e-4
        assert all(int(b) == 1 for n, b in model.named_buffers() if n.endswith("num_batches_tracked"))
    else:
        assert got["running statistics"] is None and want["running statistics"] is None


def ROW_HAS_STATS(row):
    return N.ROWS[row].get("norm", "batch") == "batch"


@pytest.mark.parametrize("CI,CO,ks,groups", CHANNELS)
def test_node_references_against_autograd(CI, CO, ks, groups):
    """conv_ref / ghost_ref against torch.autograd on a plain float64 nn.Conv2d (NCHW), grouped and ungrouped, 5 x 7 maps (odd, so that
    a transposed layout cannot pass), and the forward against the sum over taps written out."""
    g = torch.Generator().manual_seed(CI * 100 + CO)
    x = torch.randn(2, 5, 7, CI, generator=g)
    dy = torch.randn(2, 5, 7, CO, generator=g)
    conv = nn.Conv2d(CI, CO, ks, padding=ks // 2, groups=groups, bias=False).double()
    xm = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    ym = conv(xm)
    ym.backward(dy.double().permute(0, 3, 1, 2))
    y, dx, dw = N.conv_ref(x, conv.weight, dy, groups=groups, round_weight=False)
    assert N.rel(y, ym.permute(0, 2, 3, 1)) < 1e-14 and N.rel(dx, xm.grad.permute(0, 2, 3, 1)) < 1e-14 and N.rel(dw, conv.weight.grad) < 1e-14
    # the taps written out: y[p] = sum_{i,j} x[p + (i, j) - ks // 2] . w[:, :, i, j]
    xp = F.pad(x.double(), (0, 0, ks // 2, ks // 2, ks // 2, ks // 2))
    taps = torch.zeros(2, 5, 7, CO, dtype=torch.float64)
    cg = CI // groups
    for i in range(ks):
        for j in range(ks):
            win = xp[:, i: i + 5, j: j + 7]
            for gi in range(groups):
                og = CO // groups
                taps[..., gi * og: (gi + 1) * og] += win[..., gi * cg: (gi + 1) * cg] @ conv.weight[gi * og: (gi + 1) * og, :, i, j].detach().t()
    assert N.rel(y, taps) < 1e-13
    # the rounded-weight convention: the same convolution on the bf16 image of the weight
    yb = N.conv_ref(x, conv.weight, dy, groups=groups)[0]
    yb2 = N.conv_ref(x, conv.weight.detach().bfloat16().double(), dy, groups=groups, round_weight=False)[0]
    assert torch.equal(yb, yb2) and 1e-4 < N.rel(yb, y) < 1e-2
    if groups == 32:
        # ghost_ref: the 32 primary channels of a 64-channel map, copied and filtered; channels 32..63 of the input ignored
        wide = torch.cat([x, torch.randn(2, 5, 7, 32, generator=g)], dim=-1)
        dout = torch.randn(2, 5, 7, 64, generator=g)
        out, dwide, dwg = N.ghost_ref(wide, conv.weight.detach().float(), dout)
        w32 = conv.weight.detach().float()
        yr, dxr, dwr = N.conv_ref(x, w32, dout[..., 32:], groups=32, round_weight=False)
        assert torch.equal(out[..., :32], x.double()) and N.rel(out[..., 32:], yr) < 1e-14
        assert N.rel(dwide[..., :32], dout[..., :32].double() + dxr) < 1e-14 and float(dwide[..., 32:].abs().sum()) == 0.0
        assert N.rel(dwg, dwr) < 1e-14


@pytest.fixture(scope="module")
def recordings():
    """one recorded forward + backward per case, in bf16 on the CPU with the stand-in nodes (computed once, shared, left unchanged)"""
    cache = {}

    def get(row, H, W):
        if (row, H, W) not in cache:
            model, ref = N.make_models(row, H, W)
            x, gy = N.make_inputs(H, W)
            cache[(row, H, W)] = (model, ref, x, gy) + N.run_recorded(model, x, gy, conv=N.emulated_conv_nhwc, ghost=N.emulated_ghost_dw)
        return cache[(row, H, W)]
    return get


@pytest.mark.parametrize("row,H,W", N.CASES, ids=N.CASE_IDS)
def test_condition_of_the_device_test(recordings, row, H, W):
    """The seeds and shapes of the device test with every convolution input and dy rounded to bf16 (the bf16 network, its two native
    nodes replaced by torch stand-ins with the same rounding points): no node is dead -- every reference output, data gradient and
    weight gradient has a 2-norm above 1e-6 of its operands' norm product --, the routes `_compact_ok` / `p4c_conv_kernel_kind` would
    take are the stated ones (host-side dispatch code: no device), the node counts are the network's, and the stand-ins pass the
    comparison with its bars (so the bars are attainable by a one-rounding implementation)."""
    model, ref, x, gy, rec, y, dx, grads = recordings(row, H, W)
    assert x.shape == (N.B, H, W, N.CIN) and y.shape == (N.B, H, W, N.COUT) and y.dtype == torch.float32
    assert dx.shape == x.shape and all(g is not None for g in grads.values())
    convs = [r for r in rec.calls if r["kind"] == "conv"]
    ghosts = [r for r in rec.calls if r["kind"] == "ghost"]
    assert len(convs) == 13 and len(ghosts) == (12 if row == "ghost-bias" else 0)
    assert all(r["x"].dtype == torch.bfloat16 and r["dy"].dtype == torch.bfloat16 and r["w"].dtype == torch.float32 for r in rec.calls)
    assert sorted({r["x"].shape[1] for r in convs}) == sorted({H >> k for k in range(5)})
    N.check_routes(rec, row, H, W)
    for i, r in enumerate(rec.calls):
        a = N.alive(r, N.node_ref(r))
        assert min(a.values()) > N.ALIVE, (row, H, W, i, r["kind"], tuple(r["x"].shape), a)
    top = N.check_nodes(rec, f"{row} {H}x{W} (stand-ins)", verbose=False)
    assert top <= 1.0


def test_node_comparison_is_sensitive_to_a_wrong_tap(recordings):
    """The node comparison on a reference with two taps of one 3x3 weight exchanged fails every bar of that node by more than 10 x, for
    a convolution at full resolution, one at 3 x 5 and a depthwise node; and a network whose convolution reads a wrong tap fails
    `check_nodes`."""
    _, _, _, _, rec, *_ = recordings("ghost-bias", *N.GRID)
    picks = [r for r in rec.calls if r["kind"] == "conv" and r["w"].shape[-1] == 3 and r["x"].shape[1] in (48, 3)][1:4:2]
    picks += [r for r in rec.calls if r["kind"] == "ghost"][:1]
    assert len(picks) == 3
    for r in picks:
        _, dx2, dw2 = rec.rerun(r)
        good = N.node_figures(r, (r["y"], r["dx"], dw2), N.node_ref(r))
        yb, dxb, _ = N.node_ref(r, N.swap_taps(r["w"]))       # (the weight gradient does not depend on w: its own taps exchanged)
        bad = N.node_figures(r, (r["y"], r["dx"], dw2), (yb, dxb, N.swap_taps(N.node_ref(r)[2])))
        assert all(v <= bar for v, bar in good.values()), good
        for k, (v, bar) in bad.items():
            if k.endswith("max"):
                continue       # (the 2-norm figures are the ones a wrong tap is certain to move; the largest element may sit elsewhere)
            assert v >= 10 * bar, (r["kind"], tuple(r["x"].shape), k, v, bar)
    model, _ = N.make_models("nf32", 16, 16)
    x, gy = N.make_inputs(16, 16)
    wrong = lambda x_, w_: N.emulated_conv_nhwc(x_, w_, prepare=lambda w: N.swap_taps(N._bf16_weight(w)) if w.shape[-1] == 3 else N._bf16_weight(w))
    bad_rec = N.run_recorded(model, x, gy, conv=wrong, ghost=N.emulated_ghost_dw)[0]
    with pytest.raises(AssertionError, match="rel"):
        N.check_nodes(bad_rec, "wrong tap", verbose=False)


def test_bias_comparison_is_sensitive_to_a_dropped_gradient(recordings):
    """`bias_distance`: the output convolution's bias of the `bias` row has a non-trivial gradient (above 1e-2 of its weight's), the
    stand-in network sits within 1e-2 of the oracle there, and a dropped (zero) bias gradient is at distance 1 -- more than 10 x the 1.5 x
    ratio bar of the device test.  Every other convolution bias sits in front of a batch norm: its true gradient is zero (the oracle's is
    rounding noise), which is why `bias_distance` judges it against its layer's weight gradient."""
    model, ref, x, gy, rec, y, dx, grads = recordings("bias", *N.GRID)
    want = N.oracle_train_then_eval(ref, x, gy)["named"]
    got = {n: g.double() for n, g in grads.items()}
    names = N.conv_biases(got)
    assert len(names) == 13 and "outconv.bias" in names
    assert float(want["outconv.bias"].norm()) > 1e-2 * float(want["outconv.weight"].norm())
    d = N.bias_distance(got, want, "outconv.bias")
    dropped = dict(got, **{"outconv.bias": torch.zeros_like(got["outconv.bias"])})
    d0 = N.bias_distance(dropped, want, "outconv.bias")
    assert d < 1e-2 and abs(d0 - 1.0) < 1e-12 and d0 >= 10 * 1.5 * d, (d, d0)
    for n in names:
        assert n == "outconv.bias" or float(want[n].norm()) < 1e-6 * float(want[n[:-4] + "weight"].norm()), n    # true gradient: zero


@pytest.mark.parametrize("h,w,s", [(1, 1, 16), (3, 5, 16), (6, 10, 8), (12, 20, 4), (24, 40, 2), (2, 1, 2), (1, 3, 4)])
def test_upsample_bilinear_is_interpolate(h, w, s):
    """py4cast_amd.halfunet.upsample_bilinear (slices, products and sums: a fixed-order backward) against
    F.interpolate(mode="bilinear", align_corners=False) in float64, forward and adjoint, to rounding; fp32 to 1e-6.  1 x 1 and single
    rows / columns clamp every tap."""
    from py4cast_amd.halfunet import upsample_bilinear

    g = torch.Generator().manual_seed(h * 100 + w)
    a = torch.randn(2, h, w, 5, generator=g, dtype=torch.float64)
    dy = torch.randn(2, h * s, w * s, 5, generator=g, dtype=torch.float64)
    a1, a2 = a.clone().requires_grad_(True), a.clone().requires_grad_(True)
    got = upsample_bilinear(a1, s)
    ref = F.interpolate(a2.permute(0, 3, 1, 2), scale_factor=s, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert got.shape == ref.shape == dy.shape and got.is_contiguous()
    got.backward(dy)
    ref.backward(dy)
    assert N.rel(got, ref) < 1e-14 and N.rel(a1.grad, a2.grad) < 1e-14
    assert N.rel(upsample_bilinear(a.float(), s), ref) < 1e-6
