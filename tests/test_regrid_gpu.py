"""GPU parity of the regrid kernels (p4c_regrid_pack, p4c_regrid_blur through regrid.fit_to_grid and
datapipe.load_native_batch) against the float64 closed form (tests/regrid_closed_form.py) on the same fp32 sources.

Bars, un-standardised, relative to max|src|:
  * bilinear only: 1e-6.  The value is a convex combination reached in at most 5 fp32 roundings (about 3e-7); the bar is 3 x.
  * with blur: 4e-6.  Two 7-tap passes plus the blend are at most about 21 roundings (about 1.3e-6); the bar is 3 x.
A wrong convention (a half-pixel shift, ``symmetric`` for ``mirror``, the flip before the resize on an odd factor, the
sub-domain before the flip) lands above 1e-3 on the analytic field.  The shapes are the smallest at which each path can go
wrong."""

import numpy as np
import pytest
import torch

import regrid_closed_form as cf

pytestmark = pytest.mark.gpu
BILINEAR, BLUR = 1e-6, 4e-6


class Stats:
    def __init__(self, mean, std):
        self.d = {"mean": mean, "std": std}

    def to_list(self, stat, names, dtype=torch.float32):
        return self.d[stat].type(dtype)


def _check(dev, src_shape, full_size, bar, **kw):
    from py4cast_amd import regrid

    src = cf.source_field(src_shape)
    plan = regrid.RegridPlan(src_shape, full_size, **kw)
    got = regrid.fit_to_grid(src, plan, device=dev)
    want = cf.regrid(src, full_size, **kw)
    assert got.shape == want.shape == plan.out_shape and got.dtype == torch.float32 and got.device == dev
    err = np.abs(got.double().cpu().numpy() - want).max() / np.abs(src).max()
    print(f"{src_shape} -> {full_size} {kw}: {err:.3g} of max|src| (bar {bar:.0e}), blur radius {plan.radius}")
    assert err <= bar
    return plan, got


@pytest.mark.parametrize("flip", [True, False])
def test_upsampling(flip, gpu_device):
    plan, _ = _check(gpu_device, (13, 19), (37, 53), BILINEAR, subdomain=(5, 30, 7, 49), flip_lat=flip)
    assert not plan.needs_blur
    # the whole plane: the mirror at x < 0 and at x > n - 1 on both axes
    _check(gpu_device, (13, 19), (37, 53), BILINEAR, flip_lat=flip)


def test_window(gpu_device):
    _check(gpu_device, (40, 60), (90, 130), BILINEAR, window=(7, 32, 11, 51), subdomain=(3, 80, 0, 130))


def test_blur(gpu_device):
    plan, _ = _check(gpu_device, (45, 70), (18, 28), BLUR, anti_aliasing=True)
    assert plan.sigma == (0.75, 0.75) and plan.radius == (3, 3)
    # 179 x 280: more than one blur tile along both axes (16 x 64), all four edges inside the radius of some output
    _check(gpu_device, (179, 280), (72, 112), BLUR, anti_aliasing=True, subdomain=(0, 72, 100, 112))
    _check(gpu_device, (179, 280), (72, 112), BLUR, anti_aliasing=True, subdomain=(60, 72, 0, 20), flip_lat=False)
    # the blur in a window of a larger plane
    _check(gpu_device, (60, 90), (18, 28), BLUR, anti_aliasing=True, window=(9, 54, 13, 83))
    # down-sampling without the blur is another result, by far more than the bar: the blur does run
    src = cf.source_field((45, 70))
    assert np.abs(cf.regrid(src, (18, 28), anti_aliasing=True) - cf.regrid(src, (18, 28))).max() > 1e-2


def test_blur_kernel_alone(gpu_device):
    from py4cast_amd import ops, regrid

    src = cf.source_field((45, 70))
    plan = regrid.RegridPlan((45, 70), (18, 28), anti_aliasing=True)
    got = ops.regrid_blur(torch.from_numpy(np.stack([src, 2 * src])).to(gpu_device), plan.window, *regrid.device_blur_tables(plan, gpu_device))
    assert got.shape == (2, 45, 70)
    want = cf.blur(src, (18, 28))
    # two 7-tap passes of one rounding per tap and the fp32 rounding of each pass's weights: at most 16 x 2^-24 = 9.6e-7 of
    # max|src|; the bar is 2 x that.  Doubling a plane is exact in every step
    assert np.abs(got[0].double().cpu().numpy() - want).max() <= 2e-6 * np.abs(src).max()
    assert torch.equal(got[1], 2 * got[0])


def test_blur_with_several_reflections(gpu_device):
    plan, _ = _check(gpu_device, (3, 4), (1, 2), BLUR, anti_aliasing=True)
    assert plan.sigma == (1.0, 0.5) and plan.radius == (4, 2) and plan.radius[0] > plan.n[0] - 1


def test_arpege_to_1s40_has_no_blur(gpu_device):
    from py4cast_amd import _lib

    names = {}
    _lib.enable_kernel_timing(["p4c_regrid_blur", "p4c_regrid_pack"])
    try:
        plan, with_aa = _check(gpu_device, (20, 30), (50, 70), BILINEAR, anti_aliasing=True)
        names = {k: v[0] for k, v in _lib.kernel_times().items()}
    finally:
        _lib.enable_kernel_timing(None)
    assert plan.sigma == (0.0, 0.0) and not plan.needs_blur and names == {"p4c_regrid_pack": 1}          # no blur launch
    _, without = _check(gpu_device, (20, 30), (50, 70), BILINEAR)
    assert torch.equal(with_aa.view(torch.int32), without.view(torch.int32))


def test_identity(gpu_device):
    from py4cast_amd import regrid

    src = cf.source_field((25, 42))
    src[3, 5], src[10, 7] = 0.0, 1e-42                      # a zero and a denormal are copied too
    plan = regrid.RegridPlan((25, 42), (25, 42), subdomain=(2, 20, 1, 40))
    assert plan.identity and not plan.needs_blur
    got = regrid.fit_to_grid(src, plan, device=gpu_device).cpu().numpy()
    want = src[::-1][2:20, 1:40]
    assert np.array_equal(got.view(np.int32), np.ascontiguousarray(want).view(np.int32))


def test_large_indices(gpu_device):
    """Titan's real sizes: the 180 x 281 ARPEGE window onto 1791 x 2801, an 11 x 101 strip at the far corner.  A coordinate
    formed in fp32 at o = 2800 is off by about 1e-4 pixel; the field's slope of about 1 per pixel puts that at 1e-4."""
    _check(gpu_device, (200, 300), (1791, 2801), BILINEAR, window=(10, 190, 9, 290), subdomain=(1780, 1791, 2700, 2801))


@pytest.fixture(scope="module")
def batch_case(gpu_device):
    """B = 2, T = 2, sub-domain 25 x 42 (2 100 rows per plane, no multiple of 256: blocks straddle (b, t) planes and the last
    block is partial); 5 features from 3 groups (2 + 2 + 1) of three geometries -- up-sampling in a window, down-sampling with a
    blur, identity -- interleaved in io_names"""
    from py4cast_amd import regrid

    full, sub = (37, 53), (5, 30, 7, 49)
    B, T = 2, 2
    plans = [regrid.RegridPlan((20, 30), full, window=(3, 16, 5, 24), subdomain=sub),
             regrid.RegridPlan((90, 130), full, subdomain=sub, anti_aliasing=True),
             regrid.RegridPlan(full, full, subdomain=sub)]
    names = [["a0", "a1"], ["b0", "b1"], ["c0"]]
    raws = []
    for gi, (plan, ns) in enumerate(zip(plans, names)):
        planes = [cf.source_field(plan.src_shape, i0=17 * (gi + 3 * k), j0=5 * k) for k in range(len(ns) * B * T)]
        raws.append(np.stack(planes).reshape(len(ns), B, T, *plan.src_shape) * np.float32(1 + gi))
    io_names = ["b1", "a0", "c0", "a1", "b0"]
    g = torch.Generator().manual_seed(3)
    stats = Stats(torch.randn(5, generator=g) * 2, torch.rand(5, generator=g) + 0.3)
    groups = [(torch.from_numpy(r).to(gpu_device), ns, p) for r, ns, p in zip(raws, names, plans)]
    return groups, raws, io_names, stats, (B, T) + plans[0].out_shape


def test_batch_against_closed_form(batch_case, gpu_device):
    from py4cast_amd import datapipe

    groups, raws, io_names, stats, (B, T, H, W) = batch_case
    batch = datapipe.load_native_batch(groups, io_names, None, stats, num_input_steps=1, standardize=False)
    full = torch.cat([batch.inputs.tensor, batch.outputs.tensor], dim=1)
    assert full.shape == (B, T, H, W, 5)
    got = full.double().cpu().numpy()
    for c, name in enumerate(io_names):
        gi = "abc".index(name[0])
        raw, names, plan = groups[gi]
        k = names.index(name)
        bar = BLUR if plan.needs_blur else BILINEAR
        assert plan.needs_blur == (gi == 1)
        for b in range(B):
            for t in range(T):
                src = raws[gi][k, b, t]
                want = cf.regrid(src, plan.full_size, window=plan.window, subdomain=plan.subdomain, anti_aliasing=plan.anti_aliasing)
                err = np.abs(got[b, t, :, :, c] - want).max() / np.abs(src).max()
                assert err <= bar, (name, b, t, err)


def test_batch_bit_equal_to_the_unfused_route_and_on_a_rerun(batch_case, gpu_device):
    from py4cast_amd import datapipe, ops, regrid

    groups, raws, io_names, stats, (B, T, H, W) = batch_case
    batch = datapipe.load_native_batch(groups, io_names, None, stats, num_input_steps=1)
    full = torch.cat([batch.inputs.tensor, batch.outputs.tensor], dim=1)
    planes = {}
    for raw, names, plan in groups:
        fitted = regrid.fit_to_grid(raw, plan)              # (Fg, B, T, H, W), un-standardised
        assert fitted.shape == (len(names), B, T, H, W)
        planes.update({n: fitted[k] for k, n in enumerate(names)})
    unfused = ops.pack_standardize(torch.stack([planes[n] for n in io_names]), stats.d["mean"].to(gpu_device), stats.d["std"].to(gpu_device))
    assert torch.equal(full.view(torch.int32), unfused.view(torch.int32))
    again = datapipe.load_native_batch(groups, io_names, None, stats, num_input_steps=1)
    assert torch.equal(torch.cat([again.inputs.tensor, again.outputs.tensor], dim=1).view(torch.int32), full.view(torch.int32))
    assert (full.std(dim=(0, 1, 2, 3)) > 0.1).all()


def test_load_native_batch_product(batch_case, gpu_device):
    from py4cast_amd import datapipe
    from py4cast_amd.namedtensor import NamedTensor

    groups, raws, io_names, stats, (B, T, H, W) = batch_case
    forcing = NamedTensor(torch.zeros(B, T - 1, H, W, 1, device=gpu_device), datapipe.DIMS.copy(), ["f"])
    batch = datapipe.load_native_batch(groups, io_names, forcing, stats, num_input_steps=1)
    assert batch.inputs.tensor.shape == (B, 1, H, W, 5) and batch.outputs.tensor.shape == (B, T - 1, H, W, 5)
    assert batch.inputs.names == batch.outputs.names == datapipe.DIMS
    assert batch.inputs.feature_names == batch.outputs.feature_names == io_names
    assert batch.forcing is forcing and batch.num_pred_steps == T - 1
    assert batch.inputs.tensor.dtype == torch.float32 and batch.inputs.tensor.device == gpu_device
    # the same ItemBatch as load_batch on planes already fitted
    from py4cast_amd import regrid

    fitted = {n: regrid.fit_to_grid(raw, plan)[k] for raw, names, plan in groups for k, n in enumerate(names)}
    want = datapipe.load_batch(torch.stack([fitted[n] for n in io_names]), io_names, forcing, stats, num_input_steps=1)
    assert torch.equal(batch.inputs.tensor, want.inputs.tensor) and torch.equal(batch.outputs.tensor, want.outputs.tensor)


def test_nan_locality(gpu_device):
    from py4cast_amd import regrid

    src_shape, full, sub = (13, 19), (37, 53), (0, 37, 0, 53)
    plan = regrid.RegridPlan(src_shape, full, subdomain=sub)
    rt, ct = plan.row_taps, plan.col_taps
    for (i, j) in ((6, 9), (0, 0), (12, 18)):
        src = cf.source_field(src_shape)
        src[i, j] = np.nan
        got = torch.isnan(regrid.fit_to_grid(src, plan, device=gpu_device)).cpu().numpy()
        rows = (rt["i0"] == i) | (rt["i1"] == i)          # with either weight: a tap of weight 0 counts
        cols = (ct["i0"] == j) | (ct["i1"] == j)
        want = rows[:, None] & cols[None, :]
        assert want.any() and not want.all() and np.array_equal(got, want), (i, j)
    # an exact hit (f = 0 on a row): 7 -> 21 points has x = (o - 1) / 3, whole at o = 1, 4, ...; the other tap has weight 0
    plan = regrid.RegridPlan((7, 9), (21, 27), flip_lat=False)
    assert plan.row_taps["f"][4] == 0 and plan.row_taps["i0"][4] == 1 and plan.row_taps["i1"][4] == 2
    src = cf.source_field((7, 9))
    src[2, 4] = np.nan
    got = torch.isnan(regrid.fit_to_grid(src, plan, device=gpu_device)).cpu().numpy()
    assert got[4, 13] and got[4].sum() == got[5].sum() > 0 and not got[0].any()


def test_limits(gpu_device):
    from py4cast_amd import _lib, ops, regrid

    plan = regrid.RegridPlan((9, 11), (20, 26), subdomain=(2, 12, 3, 16))
    H, W = plan.out_shape
    g = torch.Generator().manual_seed(7)
    raw = torch.randn(145, 1, 2, 9, 11, generator=g).to(gpu_device)
    taps = regrid.device_taps([plan], gpu_device)
    feats = [(0, k, 0, 0, 0, 0.0, 1.0, 143 - k) for k in range(144)]           # the whole LDS tile, channels reversed
    out = ops.regrid_pack([raw], feats, taps, [plan.n], 1, 2, H, W)
    assert out.shape == (1, 2, H, W, 144)
    want = regrid.fit_to_grid(raw, plan)                                        # (145, 1, 2, H, W)
    assert torch.equal(out, want[:144].flip(0).permute(1, 2, 3, 4, 0))
    with pytest.raises(_lib.P4CError, match="at most 144"):
        ops.regrid_pack([raw], feats + [(0, 144, 0, 0, 0, 0.0, 1.0, 144)], taps, [plan.n], 1, 2, H, W)
    with pytest.raises(_lib.P4CError, match="each once"):
        ops.regrid_pack([raw], [(0, 0, 0, 0, 0, 0.0, 1.0, 1)], taps, [plan.n], 1, 2, H, W)
    with pytest.raises(_lib.P4CError, match="leaves its"):
        ops.regrid_pack([raw], [(0, 0, 1, 0, 0, 0.0, 1.0, 0)], taps, [plan.n], 1, 2, H, W)
    with pytest.raises(_lib.P4CError, match="taps"):
        ops.regrid_pack([raw], [(0, 0, 0, 0, 0, 0.0, 1.0, 0)], taps, [plan.n], 1, 2, H + 1, W)
    blur = regrid.RegridPlan((45, 70), (18, 28), anti_aliasing=True)
    ri, ci, rw, cw = regrid.device_blur_tables(blur, gpu_device)
    with pytest.raises(_lib.P4CError, match="window"):
        ops.regrid_blur(torch.zeros(44, 70, device=gpu_device), blur.window, ri, ci, rw, cw)
    with pytest.raises(_lib.P4CError, match="radius at most 64"):
        ops.regrid_blur(torch.zeros(45, 70, device=gpu_device), blur.window, ri, ci, torch.ones(131, device=gpu_device), cw)
