"""HalfUNet's non-default settings on the bf16 route (the module path of py4cast_amd/halfunet.py on the package's own convolution and
Ghost kernels): every native node of a training step against float64 on its stored operands, then the network against the float64
oracle next to the library route (the same network on torch's convolutions), the bias gradients, an auto-padded grid and the Lightning
module.  Helpers, rows, grids and bars: tests/halfunet_module_nodes.py; their device-free half: tests/test_halfunet_settings_nodes_cpu.py."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

import halfunet_module_nodes as N
from helpers import make_batch, make_dataset_info, synthetic_case

pytestmark = pytest.mark.gpu

MSE = [{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}]
RATIO = 1.5         # native distance over library-route distance (tests/test_ghost_native_gpu.py: measured 0.98 .. 1.03 there)


@pytest.mark.parametrize("row,H,W", N.CASES, ids=N.CASE_IDS)
def test_nodes_against_float64(gpu_device, row, H, W):
    """One training forward + backward (B = 2, 21 -> 12 channels, bf16) under the recorder; every conv_nhwc / ghost_dw call against
    float64 on its stored operands (the weight rounded to bf16 for the convolutions).  Output and data gradient are bf16 stores of an
    fp32 accumulation over exactly represented operands -- one rounding, at most 2^-9 of an element: 2-norm <= 3e-3 and largest deviation
    over max|ref| <= 6e-3 (tests/test_gemm_gpu.py); fp32 weight gradients <= 2e-3 (the compact-convolution test); ghost_dw 8e-3
    (test_ghost_depthwise_kernels).  No node is skipped (none is dead: test_condition_of_the_device_test).  The routes are the stated
    ones: at 48 x 80 the levels 48x80 and 24x40 take the compact row kernel where the channel counts allow and the padded launches
    meet kernel kinds 2, 1 and 0; below 24x40 and on the 16 x 16 grid (coarsest level 1 x 1) everything is a padded launch.  Gradient
    beyond the real input channels: none is handed back, the padded launch's own dx holds exact zeros there.  A second forward and
    backward from the same state is bit-identical."""
    from py4cast_amd import ops_model as OM

    dev = gpu_device
    model, _ = N.make_models(row, H, W)
    model = model.to(dev)
    state = copy.deepcopy(model.state_dict())
    x, gy = (t.to(dev) for t in N.make_inputs(H, W))
    rec, y, dx, grads = N.run_recorded(model, x, gy, forward=model)
    torch.cuda.synchronize()
    convs = [r for r in rec.calls if r["kind"] == "conv"]
    ghosts = [r for r in rec.calls if r["kind"] == "ghost"]
    assert len(convs) == 13 and len(ghosts) == (12 if row == "ghost-bias" else 0)
    assert all(r["x"].dtype == torch.bfloat16 and r["dy"].dtype == torch.bfloat16 and r["w"].dtype == torch.float32 for r in rec.calls)
    assert y.shape == (N.B, H, W, N.COUT) and dx.shape == x.shape and bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    kinds = N.check_routes(rec, row, H, W)
    print(f"{row} {H}x{W}: {sum(r['compact'] for r in convs)} compact calls, padded kernel kinds {sorted(kinds)}")
    top = N.check_nodes(rec, f"{row} {H}x{W}")
    print(f"{row} {H}x{W}: worst figure / bar {top:.3f}")
    if row == "ghost-bias":
        for r in convs[:-1]:       # 32 real outputs of a 64-row launch: the zero rows give exact zeros
            assert r["w"].shape[0] == 64 and float(r["y"][..., 32:].float().abs().sum()) == 0.0
    # the first convolution's padded launch (21 -> 32 input channels): dx of the 11 padding channels is exact zeros, the rest is what the
    # network got
    r0 = convs[0]
    assert r0["x"].shape[-1] == N.CIN and not r0["compact"]
    xp = F.pad(r0["x"], (0, 32 - N.CIN)).requires_grad_(True)
    w64 = F.pad(r0["w"], (0, 0, 0, 0, 0, 0, 0, 64 - r0["w"].shape[0]))
    y0 = OM._ConvNHWC.apply(xp, w64, "bf16")[..., : r0["w"].shape[0]]
    y0.backward(r0["dy"])
    assert torch.equal(y0.detach(), r0["y"]) and torch.equal(xp.grad[..., : N.CIN], r0["dx"])
    assert float(xp.grad[..., N.CIN:].float().abs().sum()) == 0.0
    # again from the same state
    model.load_state_dict(state)
    rec2, y2, dx2, grads2 = N.run_recorded(model, x, gy, forward=model, routes=False)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    assert set(grads) == set(grads2) and all(torch.equal(grads[n], grads2[n]) for n in grads)
    assert len(rec.calls) == len(rec2.calls)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(rec.calls, rec2.calls) for k in ("x", "y", "dy", "dx"))


@pytest.fixture(scope="module")
def oracle():
    """the float64 oracle's five quantities per row at 48 x 80, computed once and left unchanged"""
    cache = {}

    def get(row, ref, x, gy):
        if row not in cache:
            cache[row] = N.oracle_train_then_eval(ref, x, gy)
        return cache[row]
    return get


@pytest.mark.parametrize("row", list(N.ROWS))
def test_network_against_float64_next_to_the_library_route(gpu_device, monkeypatch, oracle, row):
    """48 x 80, B = 2: training forward + backward, then eval, on the native route and on the library route (`library_route`: the same
    network and bf16 maps on torch's convolutions), both against HalfUNetRef(...).double() on one state dict.  Each native distance
    (norm-wise relative: output, input gradient, parameter gradients, running statistics -- none under GroupNorm --, eval output) must be
    <= 1.5 x the library route's: the two routes store the same bf16 maps and differ in the order of fp32 sums.  The convolution biases
    (`bias`, `ghost-bias`): each one's error over max(|its float64 gradient|, 1e-2 |its layer's weight gradient|) -- a bias in front of
    a batch norm has a true gradient of zero and is judged against its weight's, as test_halfunet_yaml_settings_match_oracle does --,
    and the root mean square of these scaled distances over the row's biases holds the same 1.5 x (one bias alone is the noise of 32 or
    64 sums: its ratio scatters between 0.5 and 1.3 on EITHER side within one run, printed, not asserted); `outconv.bias` of the `bias`
    row has a non-trivial gradient (the sum of dy) and holds the ratio on its own.
    Measured on an MI355X, native / library (also in profiles/halfunet_settings_bf16.txt):
      row         output             input gradient   parameter grads  running stats        eval output
      nf32        3.193e-2/3.270e-2  0.3729/0.3638    0.3630/0.3542    1.763e-4/1.768e-4    8.886e-3/8.821e-3
      bias        3.771e-2/3.823e-2  0.4298/0.4284    0.4159/0.4151    1.983e-4/2.026e-4    3.553e-3/3.562e-3
      ghost-bias  3.654e-2/3.489e-2  0.4183/0.4234    0.4036/0.4080    1.554e-4/1.635e-4    3.869e-3/3.896e-3
      ghost-nf48  3.305e-2/3.247e-2  0.4080/0.4023    0.3884/0.3816    1.496e-4/1.375e-4    9.593e-3/9.306e-3
      group       9.509e-3/9.604e-3  0.2781/0.2943    0.1962/0.2165    (none)               9.509e-3/9.604e-3
      tanh        3.320e-2/3.363e-2  0.4444/0.4349    0.4281/0.4182    1.721e-4/1.755e-4    7.863e-3/7.921e-3
    -- ratios 0.91 ... 1.09 (the gradients of these random, untrained networks sit at 0.2 ... 0.45 from float64 on either route: bf16
    maps through twelve norms).  Convolution bias gradients, rms of the scaled distances: bias 1.180e-2/1.100e-2, ghost-bias
    0.2032/0.2261; outconv.bias 3.197e-3/3.197e-3 in both rows."""
    dev = gpu_device
    H, W = N.GRID
    native, ref = N.make_models(row, H, W)
    library = copy.deepcopy(native)
    x, gy = N.make_inputs(H, W)
    want = oracle(row, ref, x, gy)
    got_n = N.train_then_eval(native.to(dev), x, gy, dev)
    N.library_route(monkeypatch)
    got_l = N.train_then_eval(library.to(dev), x, gy, dev)
    monkeypatch.undo()
    names = [k for k in N.QUANTITIES if want[k] is not None]
    assert (len(names) == 4 and "running statistics" not in names) if row == "group" else len(names) == 5
    dist = {k: (N.rel(got_n[k], want[k]), N.rel(got_l[k], want[k])) for k in names}
    for k, (dn, dl) in dist.items():
        print(f"settings network {row}, {k}: native {dn:.4e} library {dl:.4e} ratio {dn / dl:.3f}")
    biases = N.conv_biases(want["named"])
    assert len(biases) == {"bias": 13, "ghost-bias": 25}.get(row, 0)
    bdist = {n: (N.bias_distance(got_n["named"], want["named"], n), N.bias_distance(got_l["named"], want["named"], n)) for n in biases}
    for n, (dn, dl) in bdist.items():
        print(f"settings network {row}, gradient of {n}: native {dn:.4e} library {dl:.4e} ratio {dn / dl:.3f}")
    if bdist:
        rms = [math.sqrt(sum(v[i] ** 2 for v in bdist.values()) / len(bdist)) for i in (0, 1)]
        print(f"settings network {row}, convolution bias gradients (rms of the scaled distances): native {rms[0]:.4e} library {rms[1]:.4e} "
              f"ratio {rms[0] / rms[1]:.3f}")
    assert not torch.equal(got_n["output"], got_l["output"])          # (two routes, not one route twice)
    for k, (dn, dl) in dist.items():
        assert dn <= RATIO * dl, (row, k, dn, dl)
    if bdist:
        assert rms[0] <= RATIO * rms[1], (row, rms)
    if row == "bias":
        gb, gw = want["named"]["outconv.bias"], want["named"]["outconv.weight"]
        assert float(gb.norm()) > 1e-2 * float(gw.norm())                          # judged against itself: non-trivial
        dn, dl = N.rel(got_n["named"]["outconv.bias"], gb), N.rel(got_l["named"]["outconv.bias"], gb)
        assert float(got_n["named"]["outconv.bias"].norm()) > 0.5 * float(gb.norm()) and dn <= RATIO * dl, (dn, dl)
    if row != "group":
        assert all(int(b) == 1 for n, b in native.named_buffers() if n.endswith("num_batches_tracked"))


def test_autopad(gpu_device, monkeypatch):
    """`nf32` with autopad_enabled at 40 x 72: padded to 48 x 80 (centred), run on the native route, cropped; the shape is kept and the
    output's distance from the float64 oracle (on the padded input, cropped) is <= 1.5 x the library route's.
    Measured on an MI355X: native 2.656e-2, library 2.641e-2."""
    dev = gpu_device
    H, W = 40, 72
    native, ref = N.make_models("nf32", H, W, autopad_enabled=True)
    library = copy.deepcopy(native)
    x, _ = N.make_inputs(H, W)
    top, bottom, left, right = native.padding_for(H, W)
    assert (top, bottom, left, right) == (4, 4, 4, 4)
    ref.train()
    with torch.no_grad():
        xp = F.pad(x.double(), (0, 0, left, right, top, bottom))
        want = ref(xp.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)[:, top: top + H, left: left + W]
    native, library = native.to(dev).train(), library.to(dev).train()
    xg = x.to(dev).requires_grad_(True)
    rec = N.Recorder()
    try:
        yn = native(xg)
    finally:
        rec.undo()
    assert {tuple(r["x"].shape[1:3]) for r in rec.calls} == {(48 >> k, 80 >> k) for k in range(5)}       # the padded grid, natively
    yn.float().square().mean().backward()
    assert yn.shape == (N.B, H, W, N.COUT) and xg.grad.shape == x.shape and bool(torch.isfinite(xg.grad).all())
    N.library_route(monkeypatch)
    with torch.no_grad():
        yl = library(x.to(dev))
    monkeypatch.undo()
    dn, dl = N.rel(yn, want), N.rel(yl, want)
    print(f"settings autopad output: native {dn:.4e} library {dl:.4e} ratio {dn / dl:.3f}")
    assert yl.shape == yn.shape and not torch.equal(yn, yl)
    assert dn <= RATIO * dl, (dn, dl)


@pytest.mark.parametrize("row", ["nf32", "ghost-bias"])
def test_through_the_lightning_module(gpu_device, monkeypatch, row):
    """scaled_ar, T = 2, 32 x 32, F = 12, bf16, the generic per-step rollout (the case of
    test_halfunet_yaml_settings_train_through_lightning): a finite loss, a gradient on every parameter, and the native loss within 1e-2
    relative of the library route's (the bf16 bar of tests/test_inter_steps_rollout_gpu.py).
    Measured on an MI355X, native / library: nf32 44.122093 / 44.120743, ghost-bias 44.582260 / 44.571423."""
    from py4cast_amd.lightning import AutoRegressiveLightning

    case = synthetic_case(seed=23, B=2, T=2, H=32, W=32, F=12, Ff=5, Fs=4, border=0)
    info = make_dataset_info(case, 5)

    def run():
        torch.manual_seed(31)
        lm = AutoRegressiveLightning({**N.ROWS[row], **N.BF16}, info, None, num_pred_steps_train=2, batch_size=2, model_name="HalfUNet",
                                     losses=MSE, training_strategy="scaled_ar").to(gpu_device)
        assert lm.model.module_path and not lm.model.ghost_native and lm.model.native_rollout is None
        rec = N.Recorder(routes=False)
        try:
            loss = lm.training_step(make_batch(case, gpu_device), 0)
        finally:
            rec.undo()
        loss.backward()
        assert bool(torch.isfinite(loss))
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in lm.model.parameters())
        return float(loss.detach()), len(rec.calls)

    native, ncalls = run()
    N.library_route(monkeypatch)
    library, lcalls = run()
    monkeypatch.undo()
    print(f"settings lightning {row}: loss native {native:.6f} library {library:.6f}, native node calls {ncalls}")
    assert ncalls > 0 and lcalls == 0
    assert abs(native - library) <= 1e-2 * abs(library)
