"""Regrid of native-grid planes, the parts that need no GPU: the float64 closed form (tests/regrid_closed_form.py) against the
scipy.ndimage goldens and against scipy itself, the host tables of ``py4cast_amd.regrid.RegridPlan`` against the closed form's
exact coordinates, Titan's window and blur parameters, and the refusals."""

import glob
import json
import os

import numpy as np
import pytest
import torch

import regrid_closed_form as cf

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GOLDENS = sorted(os.path.basename(f)[len("regrid_"):-len(".npz")] for f in glob.glob(os.path.join(GOLD, "regrid_*.npz")))


def _case(name):
    z = np.load(os.path.join(GOLD, f"regrid_{name}.npz"))
    kw = dict(full_size=tuple(int(v) for v in z["full_size"]), window=tuple(int(v) for v in z["window"]),
              subdomain=tuple(int(v) for v in z["subdomain"]), anti_aliasing=bool(z["anti_aliasing"]), flip_lat=bool(z["flip_lat"]))
    return tuple(int(v) for v in z["src_shape"]), kw, z["expected"]


def test_goldens_are_all_there():
    assert len(GOLDENS) == 12 and {"up_flip", "window", "down_blur", "tiny_blur", "identity", "titan_strip"} <= set(GOLDENS)


@pytest.mark.parametrize("name", GOLDENS)
def test_closed_form_equals_golden(name):
    src_shape, kw, expected = _case(name)
    got = cf.regrid(cf.source_field(src_shape), **kw)
    assert got.shape == expected.shape and got.dtype == np.float64
    d = np.abs(got - expected).max()
    print(f"{name}: closed form against scipy.ndimage {d:.3g}")
    assert d <= 1e-12


# the shapes the definition was first checked on, and the large-index strip; full planes, no flip: scipy's own output
@pytest.mark.parametrize("src,full,aa", [((13, 19), (37, 53), False), ((45, 70), (18, 28), True), ((45, 70), (18, 28), False),
                                         ((7, 9), (70, 91), True), ((52, 74), (179, 280), False), ((179, 280), (72, 112), True),
                                         ((10, 10), (10, 10), False), ((3, 4), (1, 2), True)])
def test_closed_form_equals_scipy(src, full, aa):
    ndi = pytest.importorskip("scipy.ndimage")
    img = cf.source_field(src).astype(np.float64)
    factors = np.array(src, dtype=np.float64) / np.array(full, dtype=np.float64)
    want = ndi.gaussian_filter(img, sigma=np.maximum(0, (factors - 1) / 2), mode="mirror") if aa else img
    want = ndi.zoom(want, 1 / factors, order=1, mode="mirror", grid_mode=True)
    got = cf.regrid(img, full, anti_aliasing=aa, flip_lat=False)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("name", GOLDENS)
def test_plan_tables_equal_the_closed_form_coordinates(name):
    from py4cast_amd import ops, regrid

    src_shape, kw, expected = _case(name)
    plan = regrid.RegridPlan(src_shape, **kw)
    r0, r1, c0, c1 = kw["window"]
    n = (r1 - r0, c1 - c0)
    assert plan.n == n and plan.N == kw["full_size"] and plan.out_shape == expected.shape
    assert plan.row_taps.dtype == ops.REGRID_TAP and plan.row_taps.itemsize == 16
    rows, cols = cf.output_indices(kw["full_size"], kw["subdomain"], kw["flip_lat"])
    for taps, length, N, outputs in ((plan.row_taps, n[0], plan.N[0], rows), (plan.col_taps, n[1], plan.N[1], cols)):
        i0, i1, f = cf.coordinates(length, N, outputs)
        assert np.array_equal(taps["i0"], i0) and np.array_equal(taps["i1"], i1)
        assert taps["f"].dtype == np.float32 and np.abs(taps["f"].astype(np.float64) - f).max() <= 2.0 ** -24   # f in [0, 1)
        assert (taps["i0"] >= 0).all() and (taps["i1"] <= length - 1).all() and (taps["f"] >= 0).all() and (taps["f"] < 1).all()
    assert plan.identity == (name == "identity")
    if plan.identity:
        assert (plan.row_taps["f"] == 0).all() and (plan.col_taps["f"] == 0).all() and not plan.needs_blur
        assert np.array_equal(plan.row_taps["i0"], rows) and np.array_equal(plan.col_taps["i0"], cols)
    # the blur's tables are the closed form's
    for axis in (0, 1):
        sigma, r, w = cf.gaussian(n[axis], plan.N[axis]) if kw["anti_aliasing"] else (0.0, 0, np.ones(1))
        assert plan.sigma[axis] == sigma and plan.radius[axis] == r and np.array_equal(plan.weights[axis], w)
        index = (plan.row_index, plan.col_index)[axis]
        assert index.dtype == np.int32 and np.array_equal(index, cf.mirror(np.arange(-r, n[axis] + r), n[axis]))
    assert plan.needs_blur == (name in ("down_blur", "down_blur_strip", "tiny_blur"))


def test_plans_of_equal_geometry_share_a_key():
    from py4cast_amd import regrid

    a = regrid.RegridPlan((40, 60), (90, 130), window=(7, 32, 11, 51), subdomain=(3, 80, 0, 130))
    b = regrid.RegridPlan((25, 40), (90, 130), subdomain=(3, 80, 0, 130))                      # the same 25 x 40 source, no window
    c = regrid.RegridPlan((25, 40), (90, 130), subdomain=(3, 80, 0, 130), flip_lat=False)
    assert a.key == b.key and a.key != c.key and hash(a.key) == hash(b.key)
    assert np.array_equal(a.row_taps, b.row_taps) and not np.array_equal(a.row_taps, c.row_taps)
    # the footprint: the source rows and columns the sub-domain's taps span.  Rows 1780 .. 1790 flipped are the resized rows
    # 10 .. 0: x from 0.555 down to -0.45 mirrored to 0.45, taps 0 and 1.  Columns 2700 .. 2800: x from 270.42 (tap 270) to
    # 280.45 mirrored to 279.55 (taps 279 and 280): 11 columns
    strip = regrid.RegridPlan((180, 281), (1791, 2801), subdomain=(1780, 1791, 2700, 2801))
    assert strip.footprint == (2, 11) and regrid.source_bytes(strip, 5) == 4 * 2 * 11 * 5


def test_titan_window_and_blur_parameters():
    from py4cast_amd import regrid

    grids = json.load(open(os.path.join(GOLD, "titan_grids.json")))
    assert sorted(grids) == ["ANTJP7CLIM_1S100", "PAAROME_1S100", "PAAROME_1S40", "PA_01D"]
    arp, aro = grids["PA_01D"], grids["PAAROME_1S100"]
    # a decoded GRIB's coordinates: micro-degrees as integers over 1e6, north to south
    lats = np.arange(72_000_000, 20_000_000 - 1, -100_000) / 1e6
    lons = np.arange(-32_000_000, 42_000_000 + 1, 100_000) / 1e6
    assert (len(lats), len(lons)) == tuple(arp["size"])
    w = regrid.titan_window(lats, lons, aro["extent"])
    assert (w[1] - w[0], w[3] - w[2]) == (180, 281)
    assert lats[w[0]] == 55.4 and lats[w[1] - 1] == 37.5 and lons[w[2]] == -12.0 and lons[w[3] - 1] == 16.0
    mask_lat, mask_lon = (lats >= 37.5) & (lats <= 55.4), (lons >= -12.0) & (lons <= 16.0)        # the reference's masks
    arr = np.arange(521 * 741).reshape(521, 741)
    assert np.array_equal(arr[mask_lat, :][:, mask_lon], arr[w[0]:w[1], w[2]:w[3]])
    with pytest.raises(ValueError, match="not contiguous"):
        regrid.titan_window(np.where(np.arange(521) == 200, 0.0, lats), lons, aro["extent"])
    with pytest.raises(ValueError, match="not contiguous"):
        regrid.titan_window(lats, np.concatenate([lons[:400], lons[:341]]), aro["extent"])
    with pytest.raises(ValueError, match="no latitudes"):
        regrid.titan_window(lats - 60, lons, aro["extent"])
    # PAAROME_1S100 -> PAAROME_1S40: sigma 0.749 on both axes, radius 3
    plan = regrid.RegridPlan(aro["size"], grids["PAAROME_1S40"]["size"], subdomain=(100, 612, 240, 880), anti_aliasing=True)
    assert plan.sigma == pytest.approx(((1791 / 717 - 1) / 2, (2801 / 1121 - 1) / 2), rel=1e-15)
    assert all(abs(s - 0.749) < 5e-4 for s in plan.sigma) and plan.radius == (3, 3) and plan.needs_blur
    for s, wts in zip(plan.sigma, plan.weights):
        assert wts.shape == (7,) and wts.dtype == np.float64 and abs(wts.sum() - 1) <= 1e-15 and np.array_equal(wts, wts[::-1])
        assert wts[4] / wts[3] == pytest.approx(np.exp(-0.5 / s ** 2), rel=1e-14)
    # ARPEGE -> PAAROME_1S40 asks for anti_aliasing and gets no blur: an up-sampling axis has sigma 0
    plan = regrid.RegridPlan(arp["size"], grids["PAAROME_1S40"]["size"], window=w, subdomain=(100, 612, 240, 880), anti_aliasing=True)
    assert plan.sigma == (0.0, 0.0) and plan.radius == (0, 0) and not plan.needs_blur and plan.out_shape == (512, 640)


class Stats:
    def __init__(self, n):
        self.d = {"mean": torch.zeros(n), "std": torch.ones(n)}

    def to_list(self, stat, names, dtype=torch.float32):
        return self.d[stat].type(dtype)


def test_refusals():
    from py4cast_amd import datapipe, regrid

    with pytest.raises(ValueError, match="radius 66.*at most 64"):         # sigma = (34 - 1) / 2 = 16.5, radius 66
        regrid.RegridPlan((340, 340), (10, 340), anti_aliasing=True)
    assert regrid.RegridPlan((330, 340), (10, 340), anti_aliasing=True).radius == (64, 0)
    for shape, window in (((1, 9), None), ((9, 1), None), ((9, 9), (3, 4, 0, 9)), ((9, 9), (0, 9, 5, 6))):
        with pytest.raises(ValueError, match="at least 2 points"):
            regrid.RegridPlan(shape, (20, 20), window=window)
    with pytest.raises(ValueError, match="window"):
        regrid.RegridPlan((9, 9), (20, 20), window=(0, 10, 0, 9))
    with pytest.raises(ValueError, match="sub-domain"):
        regrid.RegridPlan((9, 9), (20, 20), subdomain=(0, 21, 0, 20))
    # groups on different sub-domains, too many features, names that do not match: refused on the host, before any device work
    a = regrid.RegridPlan((9, 9), (20, 20), subdomain=(2, 12, 3, 13))
    b = regrid.RegridPlan((5, 7), (20, 20), subdomain=(3, 13, 3, 13))
    raw_a, raw_b = torch.zeros(2, 1, 2, 9, 9), torch.zeros(1, 1, 2, 5, 7)
    with pytest.raises(ValueError, match="one launch writes one sub-domain"):
        datapipe.load_native_batch([(raw_a, ["p", "q"], a), (raw_b, ["r"], b)], ["p", "q", "r"], None, Stats(3), 1)
    c = regrid.RegridPlan((5, 7), (21, 20), subdomain=(2, 12, 3, 13))        # the same indices of another full grid
    with pytest.raises(ValueError, match="one launch writes one sub-domain"):
        datapipe.load_native_batch([(raw_a, ["p", "q"], a), (raw_b, ["r"], c)], ["p", "q", "r"], None, Stats(3), 1)
    names = [f"f{i}" for i in range(145)]
    with pytest.raises(ValueError, match="at most 144"):
        datapipe.load_native_batch([(torch.zeros(145, 1, 2, 9, 9), names, a)], names, None, Stats(145), 1)
    with pytest.raises(ValueError, match="differ"):
        datapipe.load_native_batch([(raw_a, ["p", "q"], a)], ["p", "x"], None, Stats(2), 1)
    with pytest.raises(ValueError, match="is in groups"):
        datapipe.load_native_batch([(raw_a, ["p", "q"], a), (raw_a, ["q", "r"], a)], ["p", "q", "r"], None, Stats(3), 1)
    with pytest.raises(ValueError, match="is not"):
        datapipe.load_native_batch([(raw_b, ["p"], a)], ["p"], None, Stats(1), 1)


def test_regrid_has_no_cpu_path():
    from py4cast_amd import _lib, datapipe, ops, regrid

    plan = regrid.RegridPlan((9, 9), (20, 20), subdomain=(2, 12, 3, 13))
    taps = torch.zeros(1, 20, 4, dtype=torch.int32)
    with pytest.raises(_lib.P4CError):
        ops.regrid_pack([torch.zeros(1, 1, 1, 9, 9)], [(0, 0, 0, 0, 0, 0.0, 1.0, 0)], taps, [(9, 9)], 1, 1, 10, 10)
    blur = regrid.RegridPlan((45, 70), (18, 28), anti_aliasing=True)
    with pytest.raises(_lib.P4CError):
        ops.regrid_blur(torch.zeros(45, 70), blur.window, torch.from_numpy(blur.row_index), torch.from_numpy(blur.col_index),
                        torch.from_numpy(blur.weights[0]).float(), torch.from_numpy(blur.weights[1]).float())
    with pytest.raises(_lib.P4CError):
        regrid.fit_to_grid(np.zeros((9, 9), dtype=np.float32), plan)
    with pytest.raises(_lib.P4CError):
        datapipe.load_native_batch([(torch.zeros(1, 1, 2, 9, 9), ["p"], plan)], ["p"], None, Stats(1), 1)
