"""
The latency-oriented 3x3 convolution 64 -> 64 of the HalfUNet plan's coarse levels (csrc/conv_small.hip) against the kernel it
replaces there (row-streaming / ring kernel through p4c_conv_fwd), a float64 reference, a closed form, norm_finalize, and -- on the
diagnostic library, P4C_SMALL_CONV on / off -- the whole plan.  The op-level cases go through p4c_conv_small_fwd, which runs the
kernel at any shape, routed or not; what the plan routes is p4c_conv_small_ok.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, H, W): the plan levels of the benchmark, a single sample, H not a multiple of any tile height with W not a multiple of 32 and
# three samples, the Titan level-4 width, W not a multiple of 32
SHAPES = [(2, 32, 32), (2, 64, 64), (2, 128, 128), (2, 256, 256), (1, 8, 64), (3, 17, 72), (2, 5, 40), (2, 16, 80)]
MODES = ["plain", "plain+stats", "transform+stats"]


def rel_err(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


_CASES = {}


def _case(dev, B, H, W):
    """Operands of one shape and the old kernel's results on them: computed once, shared by the tests, never modified."""
    from py4cast_amd import ops_model as om

    key = (B, H, W)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * B + 10 * H + W)
        x = torch.randn(B, H, W, 64, generator=g).bfloat16().to(dev)
        w = (torch.randn(64, 64, 3, 3, generator=g) * 0.1).to(dev)
        sc = (torch.rand(B, 64, generator=g) + 0.5).to(dev)
        sh = (torch.randn(B, 64, generator=g) * 0.3).to(dev)
        wp = om.prep_weights(w, False, 64, 64, compute="bf16")
        old = {"plain": (om.conv_fwd(x, wp, 3, compute="bf16"), None),
               "plain+stats": om.conv_fwd(x, wp, 3, want_stats=True, compute="bf16"),
               "transform+stats": om.conv_fwd(x, wp, 3, in_scale=sc, in_shift=sh, in_relu=True, want_stats=True, compute="bf16")}
        _CASES[key] = dict(x=x, w=w, sc=sc, sh=sh, wp=wp, old=old)
    return _CASES[key]


def _small(c, mode, **kw):
    from py4cast_amd import ops_model as om

    tr = mode.startswith("transform")
    return om.conv_small_fwd(c["x"], c["wp"], in_scale=c["sc"] if tr else None, in_shift=c["sh"] if tr else None, **kw)


def _totals(stats, B):
    return stats.view(B, -1, 2, 64).double().sum((0, 1))   # (2, 64): sum and sum of squares per channel


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_stored_map_bit_equal_to_the_kernel_it_replaces(gpu_device, B, H, W):
    """torch.equal of the stored bf16 map with p4c_conv_fwd (row or ring kernel) on the same operands, three forward modes; the
    statistics differ in summation order only (the relative difference is printed; measured 2e-9 .. 1.7e-8 over these shapes, where
    rows against ring measured 1.5e-7).
    Seven of the eight shapes are inside the routing predicate; 2 x 256 x 256 is not (the micro-benchmark has the row kernel faster
    there: profiles/small_conv_micro.txt) -- the kernel is checked on it all the same, and that the plan falls back there is
    test_plan_falls_back_outside_the_predicate."""
    from py4cast_amd import ops_model as om

    c = _case(gpu_device, B, H, W)
    assert om.conv_small_ok(B, H, W) == ((B, H, W) != (2, 256, 256))
    for mode in MODES:
        ref, ref_stats = c["old"][mode]
        if mode == "plain":
            out, stats = _small(c, mode), None
        else:
            out, stats = _small(c, mode, want_stats=True)
        assert out.dtype == torch.bfloat16 and torch.equal(out, ref), (mode, float((out.float() - ref.float()).abs().max()))
        if stats is not None:
            d = rel_err(_totals(stats, B), _totals(ref_stats, B))
            print(f"{B}x{H}x{W} {mode}: statistics, small against the old kernel: {d:.3g}")
            assert d < 2e-5


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_against_float64_on_the_rounded_operands(gpu_device, B, H, W):
    """The project's bars: output <= 8e-3 relative with bf16 storage against a float64 convolution of the bf16-rounded operands, the
    statistics <= 2e-5 against float64 sums of the stored values."""
    c = _case(gpu_device, B, H, W)
    w64 = c["w"].bfloat16().double()
    for mode in MODES[1:]:
        xin = c["x"].float()
        if mode.startswith("transform"):
            xin = torch.relu((xin * c["sc"][:, None, None, :] + c["sh"][:, None, None, :]).bfloat16().float())
        xp = torch.nn.functional.pad(xin.double(), (0, 0, 1, 1, 1, 1))
        ref = torch.zeros(B, H, W, 64, dtype=torch.float64, device=gpu_device)
        for ky in range(3):
            for kx in range(3):
                ref += xp[:, ky:ky + H, kx:kx + W, :] @ w64[:, :, ky, kx].t()
        out, stats = _small(c, mode, want_stats=True)
        assert rel_err(out, ref) < 8e-3, mode
        assert float((out.double() - ref).abs().max()) < 0.25   # a misplaced row or column is O(1)
        o64 = out.double()
        own = torch.stack([o64.sum((0, 1, 2)), (o64 * o64).sum((0, 1, 2))])
        assert rel_err(_totals(stats, B), own) < 2e-5, mode


@pytest.mark.parametrize("H,W", [(17, 72), (6, 33), (32, 32)])
def test_all_ones_counts_the_taps_in_range(gpu_device, H, W):
    """All-ones input, every weight 1/64: each output is the number of taps inside the image -- 4 at corners, 6 at edges, 9 inside --
    exactly, for every sample of B = 3 (halo, sample-boundary and partial-tile errors that random data hides in a tolerance)."""
    from py4cast_amd import ops_model as om

    B = 3
    x = torch.ones(B, H, W, 64, dtype=torch.bfloat16, device=gpu_device)
    wp = om.prep_weights(torch.full((64, 64, 3, 3), 1.0 / 64, device=gpu_device), False, 64, 64, compute="bf16")
    out = om.conv_small_fwd(x, wp).float()
    ny = 3 - (torch.arange(H) == 0).int() - (torch.arange(H) == H - 1).int()
    nx = 3 - (torch.arange(W) == 0).int() - (torch.arange(W) == W - 1).int()
    want = (ny[:, None] * nx[None, :]).float().to(gpu_device)[None, :, :, None].expand(B, H, W, 64)
    assert torch.equal(out, want)
    assert {float(out[b, 0, 0, 0]) for b in range(B)} == {4.0} and float(out[1, 0, 1, 5]) == 6.0 and float(out[2, 1, 1, 63]) == 9.0


@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (3, 17, 72), (2, 256, 256)])
def test_in_kernel_finalize_equals_norm_finalize_on_its_slots(gpu_device, B, H, W):
    """scale / shift / mean / rstd / running statistics from the in-kernel finish against norm_finalize on the same slots: bit-equal
    (both combine the fp32 slots in float64).  A second run of everything: bit-identical."""
    from py4cast_amd import ops_model as om

    c = _case(gpu_device, B, H, W)
    g = torch.Generator().manual_seed(5)
    gamma, beta = (torch.rand(64, generator=g) + 0.5).to(gpu_device), torch.randn(64, generator=g).to(gpu_device)
    rm0, rv0 = torch.randn(64, generator=g).to(gpu_device), (torch.rand(64, generator=g) + 0.5).to(gpu_device)

    def run():
        rm, rv = rm0.clone(), rv0.clone()
        out, stats, res = _small(c, "transform+stats", finalize=dict(gamma=gamma, beta=beta, eps=1e-5, momentum=0.1, running_mean=rm,
                                                                      running_var=rv))
        return out, stats, res, rm, rv

    out, stats, res, rm, rv = run()
    assert torch.equal(out, c["old"]["transform+stats"][0])
    assert torch.equal(stats, _small(c, "transform+stats", want_stats=True)[1])   # the slots are the same with and without the finish
    rm2, rv2 = rm0.clone(), rv0.clone()
    ref = om.norm_finalize(stats, B, H * W, gamma, beta, 1e-5, 0.1, rm2, rv2)
    for name, a, b in zip(("scale", "shift", "mean", "rstd"), res, ref):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert torch.equal(rm, rm2) and torch.equal(rv, rv2)
    assert not torch.equal(rm, rm0) and bool(torch.isfinite(res[3]).all())
    again = run()
    assert torch.equal(again[0], out) and torch.equal(again[1], stats) and torch.equal(again[3], rm) and torch.equal(again[4], rv)
    for a, b in zip(again[2], res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,H,W", [(2, 32, 32), (2, 64, 64), (3, 17, 72), (2, 128, 128)])
def test_consumer_side_finish_equals_the_in_kernel_finish(gpu_device, B, H, W):
    """The level's first convolution leaves its slots and ends; the second combines them in its prologue.  What it publishes for the
    first one -- scale / shift / mean / rstd, running statistics -- equals bit for bit what that launch's own in-kernel finish
    (BatchFin) and norm_finalize write from the same slots, and its output equals a launch that reads those arrays from memory."""
    from py4cast_amd import ops_model as om

    c = _case(gpu_device, B, H, W)
    g = torch.Generator().manual_seed(9)
    gam = [(torch.rand(64, generator=g) + 0.5).to(gpu_device) for _ in range(2)]
    bet = [torch.randn(64, generator=g).to(gpu_device) for _ in range(2)]
    rm0, rv0 = torch.randn(64, generator=g).to(gpu_device), (torch.rand(64, generator=g) + 0.5).to(gpu_device)
    fin2 = dict(gamma=gam[1], beta=bet[1], eps=1e-5, momentum=0.1)
    # reference route: the first launch finishes its own statistics, the second reads scale / shift
    rm_a, rv_a = rm0.clone(), rv0.clone()
    y1, slots1, n1 = _small(c, "plain", finalize=dict(gamma=gam[0], beta=bet[0], eps=1e-5, momentum=0.1, running_mean=rm_a, running_var=rv_a))
    y2, slots2, n2 = om.conv_small_fwd(y1, c["wp"], in_scale=n1[0], in_shift=n1[1], finalize=fin2)
    rm_n, rv_n = rm0.clone(), rv0.clone()
    nf = om.norm_finalize(slots1, B, H * W, gam[0], bet[0], 1e-5, 0.1, rm_n, rv_n)

    def handoff():
        rm_b, rv_b = rm0.clone(), rv0.clone()
        y1b, slots1b = _small(c, "plain", want_stats=True)
        res = om.conv_small_fwd(y1b, c["wp"], finalize=fin2, pre=dict(slots=slots1b, gamma=gam[0], beta=bet[0], running_mean=rm_b, running_var=rv_b))
        return (y1b, slots1b) + res + (rm_b, rv_b)

    y1b, slots1b, y2b, slots2b, n2b, n1b, rm_b, rv_b = handoff()
    assert torch.equal(y1b, y1) and torch.equal(slots1b, slots1)
    for name, a, b, r in zip(("scale", "shift", "mean", "rstd"), n1b, n1, nf):
        assert torch.equal(a, b) and torch.equal(a, r), (name, float((a - b).abs().max()), float((a - r).abs().max()))
    assert torch.equal(rm_b, rm_a) and torch.equal(rv_b, rv_a) and torch.equal(rm_b, rm_n) and torch.equal(rv_b, rv_n)
    assert torch.equal(y2b, y2) and torch.equal(slots2b, slots2) and all(torch.equal(a, b) for a, b in zip(n2b, n2))
    again = handoff()
    assert torch.equal(again[2], y2b) and all(torch.equal(a, b) for a, b in zip(again[5], n1b)) and torch.equal(again[6], rm_b)


def _saved_views(saved, lay, B, H, W):
    """Raw conv outputs Y[0..11] and normalisation arrays (scale, shift, mean, rstd) of the bf16 plan's saved workspace, at the offsets
    the library reports (ops_model.halfunet_layout)."""
    n = [B * (H >> k) * (W >> k) for k in range(5)]
    lev = [i // 2 if i < 10 else 0 for i in range(12)]
    assert lay["elem_bytes"] == 2 and lay["saved_bytes"] == saved.numel()
    Y = [saved[lay["Y"][i]: lay["Y"][i] + 2 * n[lev[i]] * 64].view(torch.bfloat16) for i in range(12)]
    norms = [saved[lay["norm"][i]: lay["norm"][i] + 4 * 4 * B * 64].view(torch.float32) for i in range(12)]
    return Y, norms


def _plan_run(model, x, gy, buffers, B, H, W, env):
    """one forward + backward under the A/B switches `env`: (y, gradients, raw conv outputs, normalisation arrays)"""
    from py4cast_amd import ops_model as om

    os.environ.update(env)
    try:
        with torch.no_grad():
            for n, b in model.named_buffers():
                b.copy_(buffers[n])
        for p in model.parameters():
            p.grad = None
        y = model(x)
        node, saved = y.grad_fn, []
        while node is not None and not saved:   # (behind the channel slice and the cast to the caller's dtype: the plan's node)
            saved = [t for t in getattr(node, "saved_tensors", ()) if t.dtype == torch.uint8]
            node = node.next_functions[0][0] if node.next_functions else None
        Y, norms = _saved_views(saved[0].clone(), om.halfunet_layout(model._desc(B, H, W)), B, H, W)
        (y * gy).sum().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}, Y, norms
    finally:
        for k in env:
            os.environ.pop(k, None)


def _plan_model(dev, B, H, W, cin=69, cout=60):
    from py4cast_amd.halfunet import HalfUNetMI355X, HalfUNetSettings

    torch.manual_seed(0)
    model = HalfUNetMI355X(cin, cout, (H, W), HalfUNetSettings(compute_dtype="bf16", activation_dtype="bf16")).to(dev).train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, H, W, cin, generator=g).to(dev)
    gy = torch.randn(B, H, W, cout, generator=g).to(dev)
    return model, x, gy, {n: b.clone() for n, b in model.named_buffers()}


def test_plan_falls_back_outside_the_predicate(gpu_device, diag_library):
    """2 x 256 x 256 is outside p4c_conv_small_ok (only the measured threshold excludes it: with P4C_SMALL_CONV_MAX_PIXELS raised it is
    inside).  A plan whose level 0 has that shape runs blocks 0 and 1 on the row kernel whatever the switch says: their raw outputs AND
    their statistics -- which another kernel would sum in another order -- are bit-equal with P4C_SMALL_CONV on and off."""
    from py4cast_amd import ops_model as om

    B, H, W = 2, 256, 256
    assert not om.conv_small_ok(B, H, W) and om.conv_small_ok(B, H // 2, W // 2)
    os.environ["P4C_SMALL_CONV_MAX_PIXELS"] = str(B * H * W)
    try:
        assert om.conv_small_ok(B, H, W)
    finally:
        os.environ.pop("P4C_SMALL_CONV_MAX_PIXELS", None)
    model, x, gy, buffers = _plan_model(gpu_device, B, H, W)
    on, off = (_plan_run(model, x, gy, buffers, B, H, W, {"P4C_SMALL_CONV": sw}) for sw in ("1", "0"))
    for i in (0, 1):
        assert torch.equal(on[2][i], off[2][i]) and torch.equal(on[3][i], off[3][i]), i
    assert torch.equal(on[2][2], off[2][2])   # block 2 (128 x 128, routed): equal inputs, bit-equal map


def test_plan_with_and_without_the_small_kernel(gpu_device, diag_library):
    """B = 2, 128 x 128, C_in = 69 (levels 128 .. 8): one forward + backward of the plan with P4C_SMALL_CONV on and off.  Block 0 (96
    padded input channels) is outside the kernel's reach and falls back on both routes; every 64-channel block is routed.  Block by
    block in plan order the saved raw conv output is bit-equal as long as everything before it was (the chain stops at the first block
    whose statistics -- summed in another order -- differ in a bit); the network output and every parameter gradient agree within the
    bars tests/test_model_gpu.py applies to the bf16 flavour; reruns are bit-identical."""
    from py4cast_amd import ops_model as om

    B, H, W = 2, 128, 128
    model, x, gy, buffers = _plan_model(gpu_device, B, H, W)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)

    def run(switch):
        os.environ["P4C_SMALL_CONV"] = switch
        try:
            assert om.conv_small_ok(B, H >> 1, W >> 1) == (switch == "1")
        finally:
            os.environ.pop("P4C_SMALL_CONV", None)
        return _plan_run(model, x, gy, buffers, B, H, W, {"P4C_SMALL_CONV": switch})

    on, off, on2 = run("1"), run("0"), run("1")
    # the statistics hand-off between the two convolutions of a level (P4C_SMALL_HANDOFF=0: every launch finishes its own) changes no bit
    solo = _plan_run(model, x, gy, buffers, B, H, W, {"P4C_SMALL_CONV": "1", "P4C_SMALL_HANDOFF": "0"})
    assert torch.equal(solo[0], on[0]) and all(torch.equal(a, b) for a, b in zip(solo[2] + solo[3], on[2] + on[3]))
    assert all(torch.equal(solo[1][n], on[1][n]) for n in on[1])
    bufs = {n: b.clone() for n, b in model.named_buffers()}
    _plan_run(model, x, gy, buffers, B, H, W, {"P4C_SMALL_CONV": "1"})
    assert all(torch.equal(b, bufs[n]) for n, b in model.named_buffers())   # running statistics too
    assert torch.equal(on[0], on2[0]) and all(torch.equal(on[1][n], on2[1][n]) for n in on[1])
    assert all(torch.equal(a, b) for a, b in zip(on[2], on2[2])) and all(torch.equal(a, b) for a, b in zip(on[3], on2[3]))
    compared = 0
    for i in range(12):
        assert torch.equal(on[2][i], off[2][i]), f"raw output of block {i}"
        compared += 1
        if not torch.equal(on[3][i], off[3][i]):
            break
    print("blocks compared bit for bit before the statistics first differed:", compared)
    assert compared >= 2   # block 0 (fallback on both routes) and block 1 (routed) at the least
    assert rel_err(on[0], off[0]) < 0.1
    for n in on[1]:
        a, b = on[1][n].double().flatten(), off[1][n].double().flatten()
        assert float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.85, n
