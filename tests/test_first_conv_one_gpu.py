"""The first convolution of the bf16 HalfUNet plan at 65..72 input channels in ONE launch of the row-streaming kernel (csrc/conv_rows.hip,
THIN: the loaders keep the ninth channel octet in the pad slot of the LDS pixels, the matrix waves add its K slices to the rolling
accumulators, y = bf16(fp32 sum over all channels) is rounded and written once and the statistics come from the row kernel's drain;
replaces row launch + tail pass of mfai's first Conv2d, py4cast/lightning.py:591-596): against float64 on the same bf16 operands, the
statistics against the stored map, closed-form borders, the two-launch form, and the plan with the route switched on and off.

Geometry: a workgroup owns R = H / nseg (+ 1 for the first H % nseg segments) output rows of a 64-column strip; the row loop is unrolled by
three, so R mod 3 = 0 / 1 / 2 and segments with and without the extra row are separate paths.  Small maps get two- and three-row segments
from the product geometry; the other cases force the segment count (P4C_ROWS_NSEG, diagnostic library)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

# B, H, W, cin, x_cs, forced nseg (None: the product geometry) -> rows per segment
CASES = [
    (1, 35, 64, 69, 96, 4),       # 9, 9, 9, 8: R mod 3 = 0 and 2, with and without the extra row; one strip
    (2, 13, 128, 65, 72, 3),      # 5, 4, 4: R mod 3 = 2 and 1; two strips, 144-byte source pixels
    (1, 12, 192, 72, 96, 2),      # 6, 6: R mod 3 = 0, no extra row; three strips, a full octet
    (2, 9, 64, 69, 72, None),     # 3, 2, 2, 2 (small map: two-row segments)
    (1, 8, 128, 72, 72, 1),       # 8: one segment, the strip's first and last interval are the same two
    (2, 16, 192, 65, 96, None),   # 2 x 8 segments, a single channel beyond 64
    (1, 24, 96, 70, 96, 1),       # 24: six intervals; the second strip is half outside the image
]
HALF_ULP_OF_MAX = 4e-3            # the single-op bar of tests/test_first_conv_gpu.py: half a bf16 ulp of the largest value


def _bf(t):
    return t.to(torch.bfloat16)


def _operands(B, H, W, cin, x_cs, seed, positive=False):
    """x with NaN-free garbage in the padding channels (they must meet zero weights), w at the scale of the plan's initialisation"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, x_cs, generator=g)
    x[..., cin:] = 3.0 + 100.0 * torch.rand(B, H, W, x_cs - cin, generator=g)
    w = torch.randn(64, cin, 3, 3, generator=g) * 0.2
    if positive:
        x, w = x.abs(), w.abs()
    return _bf(x), w


def _conv64(xb, w, lo, hi):
    """float64 convolution of channels lo..hi-1 of the bf16 map with the bf16-rounded weights -> (B, H, W, 64)"""
    return Fn.conv2d(xb[..., lo:hi].double().permute(0, 3, 1, 2), _bf(w)[:, lo:hi].double(), padding=1).permute(0, 2, 3, 1)


def _run(name, dev, xb, w, cin, slots_fn, stats=True):
    from py4cast_amd import _lib as L

    B, H, W, x_cs = xb.shape
    xd, wd = xb.to(dev), w.to(dev)
    y = torch.full((B, H, W, 64), float("nan"), dtype=torch.bfloat16, device=dev)
    st = None
    if stats:
        st = torch.full((B, getattr(L.lib(), slots_fn)(B, H, W), 2, 64), float("nan"), device=dev)
    L.call(name, L.ptr(xd), x_cs, cin, L.ptr(wd), L.ptr(y), L.ptr(st), B, H, W, L.stream(dev))
    torch.cuda.synchronize()
    return y.cpu(), (st.cpu() if stats else None)


def _ulps_apart(a, b):
    """|a - b| in bf16 steps of the larger magnitude (both bf16)"""
    a, b = a.double(), b.double()
    mag = torch.maximum(a.abs(), b.abs()).clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    return (a - b).abs() / ulp


@pytest.mark.parametrize("B,H,W,cin,x_cs,nseg", CASES)
def test_one_launch_against_float64(gpu_device, diag_library, monkeypatch, B, H, W, cin, x_cs, nseg):
    """y = bf16(sum over all cin channels): within half a bf16 ulp of the largest value of the float64 sum on the same bf16 operands --
    image borders, strip borders, every row-loop path; garbage in the padding channels ignored; channel sums / sums of squares of the
    STORED map within the bar of the other statistics tests (rtol 1e-5); reruns bit-identical; same map without a statistics buffer."""
    if nseg is not None:
        monkeypatch.setenv("P4C_ROWS_NSEG", str(nseg))
    xb, w = _operands(B, H, W, cin, x_cs, seed=1000 * B + 10 * H + cin)
    ref = _conv64(xb, w, 0, cin)
    y, st = _run("p4c_first_conv_one", gpu_device, xb, w, cin, "p4c_first_conv_one_slots")
    assert bool(torch.isfinite(y.float()).all())
    got = y.double()
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"one-launch vs float64: max |err| / max |ref| = {err:.3e}")
    assert err < HALF_ULP_OF_MAX, err
    # nearly always THE rounding of the float64 sum (fp32 accumulation of 9 * cin exact products), else one bf16 step away -- the bars of
    # the tail's test; the step is taken relative to max(|ref|, 1e-3): where the channels cancel to almost nothing, the fp32 noise of
    # the partial sums (1e-7 of THEIR size) is several steps of the tiny result
    share = float((y != _bf(ref)).float().mean())
    step = float(((got - _bf(ref).double()).abs() / ref.abs().clamp_min(1e-3)).max())
    print(f"share of elements that are not the rounding of the float64 sum: {share:.3e}, largest step {step:.3e}")
    assert share < 2e-3 and step < 1e-2
    s = st.double().sum(1)
    np.testing.assert_allclose(s[:, 0].numpy(), got.sum((1, 2)).numpy(), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(s[:, 1].numpy(), (got ** 2).sum((1, 2)).numpy(), rtol=1e-5, atol=1e-3)
    y2, st2 = _run("p4c_first_conv_one", gpu_device, xb, w, cin, "p4c_first_conv_one_slots")
    assert torch.equal(y, y2) and torch.equal(st, st2)
    y3, _ = _run("p4c_first_conv_one", gpu_device, xb, w, cin, "p4c_first_conv_one_slots", stats=False)
    assert torch.equal(y, y3)


@pytest.mark.parametrize("B,H,W,cin,x_cs,nseg", CASES)
def test_one_launch_against_two_launches(gpu_device, diag_library, monkeypatch, B, H, W, cin, x_cs, nseg):
    """Row launch + tail rounds y twice: y2 = bf16(bf16(a) + b) against y1 = bf16(a + b), a / b the products of channels 0..63 / beyond.  On
    NON-NEGATIVE operands |a + b| >= |a|, so the values before the last rounding differ by at most half a bf16 ulp of |y| (+ the fp32
    accumulation noise, 1e-5 of an ulp) and the stored values by at most one bf16 step -- a condition, not a statistic: the count of
    elements further apart must be 0, for the float64 model of the two forms (CPU) and for the kernels."""
    if nseg is not None:
        monkeypatch.setenv("P4C_ROWS_NSEG", str(nseg))
    xb, w = _operands(B, H, W, cin, x_cs, seed=77 + H + cin, positive=True)
    a, b = _conv64(xb, w, 0, 64), _conv64(xb, w, 64, cin)
    assert int((_ulps_apart(_bf(a + b), _bf(_bf(a).double() + b)) > 1.0).sum()) == 0     # the float64 model on the CPU
    y1, s1 = _run("p4c_first_conv_one", gpu_device, xb, w, cin, "p4c_first_conv_one_slots")
    y2, s2 = _run("p4c_first_conv_two", gpu_device, xb, w, cin, "p4c_first_conv_tail_slots")
    steps = _ulps_apart(y1, y2)
    print(f"one vs two launches: {float((steps > 0).float().mean()):.3e} of the elements differ, max {float(steps.max())} steps")
    assert int((steps > 1.0).sum()) == 0
    # one rounding is not further from float64 than two
    e1, e2 = float((y1.double() - (a + b)).norm()), float((y2.double() - (a + b)).norm())
    print(f"|y - float64|: one launch {e1:.6e}, two launches {e2:.6e}")
    assert e1 <= e2 * (1 + 1e-6)
    # the statistics are those of two non-negative maps whose elements are at most one step (2^-7 relative) apart
    t1, t2 = s1.double().sum(1).numpy(), s2.double().sum(1).numpy()
    np.testing.assert_allclose(t1[:, 0], t2[:, 0], rtol=2.0 ** -7, atol=1e-3)
    np.testing.assert_allclose(t1[:, 1], t2[:, 1], rtol=2.0 ** -6, atol=1e-3)


@pytest.mark.parametrize("B,H,W,cin,x_cs,nseg", CASES)
def test_one_launch_against_two_launches_on_signed_operands(gpu_device, diag_library, monkeypatch, B, H, W, cin, x_cs, nseg):
    """The same comparison where the products of channels 0..63 (a) and of the octet (b) may cancel.  There the second rounding of the
    two-launch form is half a step of |a|, not of |y|: |y1 - y2| <= ulp(y) / 2 + ulp(a) / 2 + ulp(y) / 2, and both lie on the grid of
    ulp(y) -- at most ONE step of u = ulp(max(|y|, |bf16(a)|)) whether ulp(y) = u or <= u / 2.  So the step is taken relative to
    max(|y|, |bf16(a)|), a per element from float64 on the CPU; the count of elements further apart must be 0 for the float64 model of
    the two forms (checked here first) and for the kernels.  (In steps of |y| alone no seed passes: the float64 model itself has 1.5-4 % of
    the elements of these cases further than one step apart.)"""
    if nseg is not None:
        monkeypatch.setenv("P4C_ROWS_NSEG", str(nseg))
    xb, w = _operands(B, H, W, cin, x_cs, seed=4242 + H + cin)
    a, b = _conv64(xb, w, 0, 64), _conv64(xb, w, 64, cin)
    floor = _bf(a).double().abs()

    def steps_with_floor(u, v):
        mag = torch.maximum(torch.maximum(u.double().abs(), v.double().abs()), floor).clamp_min(2.0 ** -126)
        return (u.double() - v.double()).abs() / torch.exp2(torch.floor(torch.log2(mag)) - 7)

    assert int((steps_with_floor(_bf(a + b), _bf(_bf(a).double() + b)) > 1.0).sum()) == 0     # the float64 model on the CPU
    y1, _ = _run("p4c_first_conv_one", gpu_device, xb, w, cin, "p4c_first_conv_one_slots", stats=False)
    y2, _ = _run("p4c_first_conv_two", gpu_device, xb, w, cin, "p4c_first_conv_tail_slots", stats=False)
    steps = steps_with_floor(y1, y2)
    print(f"signed operands, one vs two launches: {float((steps > 0).float().mean()):.3e} of the elements differ, max {float(steps.max())} steps")
    assert int((steps > 1.0).sum()) == 0
    e1, e2 = float((y1.double() - (a + b)).norm()), float((y2.double() - (a + b)).norm())
    print(f"|y - float64|: one launch {e1:.6e}, two launches {e2:.6e}")
    assert e1 <= e2 * (1 + 1e-6)


@pytest.mark.parametrize("W", [64, 128, 192])
def test_closed_form_borders_of_the_thin_taps(gpu_device, W):
    """A constant ninth octet and ONE non-zero tap weight on it (channels 0..63 of x are garbage that meets zero weights): the output is
    (cin - 64) where the tap's source pixel lies inside the image and exactly 0 where it falls on the zero padding -- at the image border,
    not at strip borders (columns 63 | 64, 127 | 128) or segment borders."""
    B, H, cin, x_cs = 1, 11, 69, 96
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, W, x_cs, generator=g)
    x[..., 64:] = 1.0
    xb = _bf(x)
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    for ky in range(3):
        for kx in range(3):
            w = torch.zeros(64, cin, 3, 3)
            w[:, 64:, ky, kx] = 1.0
            y, st = _run("p4c_first_conv_one", gpu_device, xb, w, cin, "p4c_first_conv_one_slots")
            inside = ((ys + ky - 1 >= 0) & (ys + ky - 1 < H) & (xs + kx - 1 >= 0) & (xs + kx - 1 < W)).float() * (cin - 64)
            want = inside.view(1, H, W, 1).expand(B, H, W, 64)
            assert torch.equal(y.float(), want), (ky, kx)
            assert torch.equal(st.double().sum(1)[:, 0], want.double().sum((1, 2)))
    # and one tap of a channel below 64 beside one of the octet: the two products do not mix
    w = torch.zeros(64, cin, 3, 3)
    w[:, 3, 0, 2] = 1.0
    w[:, 66, 2, 0] = 2.0
    x = torch.zeros(B, H, W, x_cs)
    x[..., 3] = 1.0
    x[..., 66] = 1.0
    y, _ = _run("p4c_first_conv_one", gpu_device, _bf(x), w, cin, "p4c_first_conv_one_slots", stats=False)
    want = ((ys - 1 >= 0) & (xs + 1 < W)).float() + 2.0 * ((ys + 1 < H) & (xs - 1 >= 0)).float()
    assert torch.equal(y.float(), want.view(1, H, W, 1).expand(B, H, W, 64))


def test_entry_point_refuses_what_it_does_not_cover(gpu_device):
    from py4cast_amd import _lib as L

    x = torch.zeros(1, 16, 64, 96, dtype=torch.bfloat16, device=gpu_device)
    w = torch.zeros(64, 69, 3, 3, device=gpu_device)
    y = torch.zeros(1, 16, 64, 64, dtype=torch.bfloat16, device=gpu_device)
    for x_cs, cin, H, W in [(96, 64, 16, 64), (96, 73, 16, 64), (64, 69, 16, 64), (96, 69, 16, 32), (96, 69, 4, 64)]:
        with pytest.raises(L.P4CError):
            L.call("p4c_first_conv_one", L.ptr(x), x_cs, cin, L.ptr(w), L.ptr(y), None, 1, H, W, L.stream(gpu_device))


def test_plan_on_the_one_launch_route_tracks_the_two_launch_plan(gpu_device, diag_library, monkeypatch):
    """Forward + backward of the native plan at 2 x 64 x 64, 69 -> 60 channels, with the first convolution in one launch (default) and as
    row launch + tail (P4C_FIRST_CONV_ONE=0, diagnostic library): the saved Y[0] of the one-launch route obeys the single-op bound against
    float64 on the operands the kernel saw, every saved map of the later blocks and the output lie within the bf16 flavour's plan bar
    (8e-2, tests/test_first_conv_gpu.py) of the other route's, every gradient points the same way (the bars of that test), reruns are
    bit-identical."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import halfunet_nodes as hn
    from py4cast_amd.halfunet import HalfUNetMI355X, HalfUNetSettings

    B, H, W = 2, 64, 64
    torch.manual_seed(0)
    model = HalfUNetMI355X(69, 60, (H, W), HalfUNetSettings(compute_dtype="bf16", activation_dtype="bf16")).to(gpu_device).train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, H, W, 69, generator=g).to(gpu_device)
    gy = torch.randn(B, H, W, 60, generator=g).to(gpu_device)

    def run(one):   # (train mode: the running statistics move from run to run and enter nothing that is compared)
        monkeypatch.setenv("P4C_FIRST_CONV_ONE", "1" if one else "0")
        return hn.run_plan(model, x, gy)

    r1, r1b, r2 = run(True), run(True), run(False)
    assert all(torch.equal(a, b) for a, b in zip(r1.Y, r1b.Y)) and all(torch.equal(a, b) for a, b in zip(r1.grads, r1b.grads))
    assert torch.equal(r1.y, r1b.y) and torch.equal(r1.dx, r1b.dx)
    w0 = next(p for n, p in model.named_parameters() if p.dim() == 4 and p.shape[1] == 69).detach().cpu()
    ref0 = _conv64(r1.x.cpu(), w0, 0, 69)
    err = float((r1.Y[0].double().cpu() - ref0).abs().max() / ref0.abs().max())
    err2 = float((r2.Y[0].double().cpu() - ref0).abs().max() / ref0.abs().max())
    print(f"Y[0] vs float64: one launch {err:.3e}, two launches {err2:.3e}")
    assert err < HALF_ULP_OF_MAX, err
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())   # noqa: E731
    cos = lambda a, b: float(torch.dot(a.double().flatten(), b.double().flatten()) / (a.double().norm() * b.double().norm()))   # noqa: E731
    for i in range(1, len(r1.Y)):
        d = rel(r1.Y[i], r2.Y[i])
        print(f"Y[{i}] one vs two launches: {d:.3e}")
        assert d < 8e-2, (i, d)
    assert rel(r1.y, r2.y) < 8e-2
    for i, (a, b) in enumerate(zip(r1.grads, r2.grads)):
        assert cos(a, b) > 0.8, i
    assert cos(torch.cat([a.flatten() for a in r1.grads]), torch.cat([b.flatten() for b in r2.grads])) > 0.9
    assert cos(r1.dx, r2.dx) > 0.9


def test_the_product_library_runs_one_launch_for_block_0_of_the_bench_shape(gpu_device):
    """2 x 512 x 512, 69 -> 60 channels, bf16: the product library (no switches) enqueues exactly ONE kernel for the first convolution per
    model call (p4c_first_conv_launch_count, counted at the launch sites of the one-launch kernel, the row launch on wide pixels and the
    tail: row launch + tail would count two), and the statistics slots of that launch fit the plan's."""
    from py4cast_amd import _lib as L
    from py4cast_amd.halfunet import HalfUNetMI355X, HalfUNetSettings

    lib = L.lib()
    assert lib.p4c_first_conv_one_slots(2, 512, 512) <= 1024
    m = HalfUNetMI355X(69, 60, (512, 512), HalfUNetSettings(compute_dtype="bf16", activation_dtype="bf16")).to(gpu_device).train()
    x = torch.randn(2, 512, 512, 69, generator=torch.Generator().manual_seed(1)).to(gpu_device)
    before = lib.p4c_first_conv_launch_count()
    with torch.no_grad():
        y = m(x)
    torch.cuda.synchronize()
    assert lib.p4c_first_conv_launch_count() - before == 1
    assert bool(torch.isfinite(y).all())
