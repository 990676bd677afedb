"""
``ops.pack_convert`` (kernel ``p4c_pack_convert``) against its numpy restatement ``pack_convert_reference``, bit for bit: every
source dtype, both load paths (16 bytes per lane where W and the strides allow it, one element otherwise), the feature counts
at which the rows per pass change, planes at a pitch, the special values of every format, a second loop trip, and the
refusals before any launch.
"""
import numpy as np
import pytest
import torch

import pack_convert_reference as R

pytestmark = pytest.mark.gpu

SHAPES = ((5, 7), (33, 47), (64, 64))
# (flip, floor, div, mul): all eight combinations
COMBOS = [(flip, floor, div, mul) for flip in (False, True) for floor in (None, 0.0) for (div, mul) in ((1.0, 1.0), (100.0, 12.0))]


def make_planes(dtype, shape, rng):
    """values of ``shape`` in ``dtype`` with the cases each format can get wrong"""
    dt = np.dtype(dtype)
    n = int(np.prod(shape))
    if dt.kind in "ui":
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, size=n, endpoint=True, dtype=np.int64)
        # the ends of the range, values under the floor, above 32767 (u16) and above 2^24 whose conversion rounds (i32)
        special = [info.min, info.max, 0, 1, info.max // 2 + 1, info.max - 1]
        if dt.kind == "i":
            special += [-1, -100, info.min + 1]
        if dt.itemsize == 4:
            special += [(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, (1 << 25) + 2, (1 << 25) + 6, (1 << 30) + 64, 2147483583]
        a[:len(special)] = special[:n]
        return a.astype(dt).reshape(shape)
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, size=n)).astype(np.float64)
    special = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, -1e-3, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 6.0e-8, 1e-40, 65504.0, -65504.0, 1e39,
               3.4028235677973366e38]
    a[:len(special)] = special[:n]
    with np.errstate(all="ignore"):
        return a.astype(dt).reshape(shape)


def to_device(a, dev):
    """numpy -> device tensor of the same bits (uint16 goes through int16: the bits are what matters)"""
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).to(dev).view(torch.uint16)
    return torch.from_numpy(a.copy()).to(dev)


def run_case(dev, dtype, F, B, T, H, W, rot, rng, pitch=False, stacked=False):
    from py4cast_amd import ops

    planes = [make_planes(dtype, (B, T, H, W), rng) for _ in range(F)]
    mean = rng.standard_normal(F).astype(np.float32)
    std = (0.5 + rng.random(F)).astype(np.float32)
    channels = rng.permutation(F)
    if stacked:
        sources = [to_device(np.stack(planes), dev)]
        where = [(0, i) for i in range(F)]
    elif pitch:      # one step more than is read: the batch stride is larger than the dense one
        sources = []
        for p in planes:
            wide = np.zeros((1, B, T + 1, H, W), dtype=p.dtype)
            wide[0, :, :T] = p
            sources.append(to_device(wide, dev)[:, :, :T])
        where = [(i, 0) for i in range(F)]
    else:
        sources = [to_device(p[None], dev) for p in planes]
        where = [(i, 0) for i in range(F)]
    feats, ref_feats = [], [None] * F
    for i in range(F):
        flip, floor, div, mul = COMBOS[(i + rot) % len(COMBOS)]
        feats.append((*where[i], floor, div, mul, flip, float(mean[i]), float(std[i]), int(channels[i])))
        ref_feats[channels[i]] = dict(floor=floor, div=div, mul=mul, flip=flip, mean=mean[i], std=std[i])
    ordered = [None] * F
    for i in range(F):
        ordered[channels[i]] = planes[i]
    _, vec = ops.convert_features(sources, feats, B, T, H, W)
    got = ops.pack_convert(sources, feats, B, T, H, W)
    assert got.shape == (B, T, H, W, F) and got.dtype == torch.float32
    R.assert_bit_equal(got.cpu().numpy(), R.pack_convert_reference(ordered, ref_feats),
                       f"{dtype} F={F} B={B} T={T} {H}x{W} rot={rot} pitch={pitch} stacked={stacked} vec={vec}")
    return vec


@pytest.mark.parametrize("F", (1, 3, 21, 144))
@pytest.mark.parametrize("dtype", R.NP_DTYPES)
def test_bit_equal_to_the_reference(gpu_device, dtype, F):
    rng = np.random.default_rng(1000 * R.NP_DTYPES.index(dtype) + F)
    paths = set()
    for (H, W) in SHAPES:
        for (B, T) in ((1, 1), (2, 3)):
            for rot in (range(len(COMBOS)) if F < len(COMBOS) else (0,)):
                paths.add(run_case(gpu_device, dtype, F, B, T, H, W, rot, rng))
    assert paths == {False, True}      # 64 x 64 loads 16 bytes per lane, the odd widths one element


@pytest.mark.parametrize("dtype", R.NP_DTYPES)
def test_planes_at_a_pitch_and_stacked_sources(gpu_device, dtype):
    rng = np.random.default_rng(7)
    for (H, W) in SHAPES:
        run_case(gpu_device, dtype, 3, 2, 3, H, W, 3, rng, pitch=True)
    assert run_case(gpu_device, dtype, 5, 2, 3, 64, 64, 1, rng, stacked=True)


@pytest.mark.parametrize("dtype,F,vec", (("<i2", 9, False), ("<f4", 21, True), ("u1", 1, True)))
def test_second_loop_trip(gpu_device, dtype, F, vec):
    """a grid large enough that the busiest workgroup makes a second pass, sized from the launch arithmetic"""
    from py4cast_amd import _lib as L

    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    assert L.lib().p4c_pack_convert_rows(F) == R.rows_per_pass(F) and L.lib().p4c_pack_convert_max_blocks() == cus * R.BLOCKS_PER_CU
    side = R.two_trip_side(F, 1, cus, multiple_of=16 if vec else 1)
    if not vec and side % 2 == 0:
        side += 1
    assert R.trips(side * side, F, cus) == 2
    assert run_case(gpu_device, dtype, F, 1, 1, side, side, 5, np.random.default_rng(11)) == vec


def test_equals_pack_standardize_without_transform(gpu_device):
    from py4cast_amd import ops

    rng = np.random.default_rng(3)
    for (H, W) in SHAPES:
        F, B, T = 21, 2, 3
        raw = torch.from_numpy(make_planes("<f4", (F, B, T, H, W), rng)).to(gpu_device)
        mean = torch.from_numpy(rng.standard_normal(F).astype(np.float32))
        std = torch.from_numpy((0.5 + rng.random(F)).astype(np.float32))
        feats = [(i, 0, None, 1.0, 1.0, False, float(mean[i]), float(std[i]), i) for i in range(F)]
        got = ops.pack_convert([raw[i:i + 1].clone() for i in range(F)], feats, B, T, H, W)
        want = ops.pack_standardize(raw, mean.to(gpu_device), std.to(gpu_device))
        R.assert_bit_equal(got.cpu().numpy(), want.cpu().numpy(), f"{H}x{W}")


def test_refusals_before_any_launch(gpu_device):
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    H, W = 8, 16
    one = torch.zeros(1, 1, 1, H, W, dtype=torch.int16, device=gpu_device)
    feat = (0, 0, None, 1.0, 1.0, False, 0.0, 1.0, 0)
    with pytest.raises(L.P4CError, match="145 features"):
        ops.pack_convert([one], [(0, 0, None, 1.0, 1.0, False, 0.0, 1.0, i) for i in range(145)], 1, 1, H, W)
    flat = torch.zeros(H * W + 8, dtype=torch.int16, device=gpu_device)
    with pytest.raises(L.P4CError, match="16-byte boundary"):
        ops.pack_convert([flat[1:1 + H * W].view(1, 1, 1, H, W)], [feat], 1, 1, H, W)
    with pytest.raises(L.P4CError, match="rows"):          # 2^31 rows by arithmetic: nothing of that size is allocated
        ops.pack_convert([one], [feat], 1 << 15, 1 << 4, 64, 64)
    with pytest.raises(L.P4CError, match="channels"):
        ops.pack_convert([one], [feat[:-1] + (1,)], 1, 1, H, W)
    with pytest.raises(L.P4CError, match="dtype"):
        ops.pack_convert([one.to(torch.int64)], [feat], 1, 1, H, W)
    # the entry point itself refuses the same, with the error code and no launch
    lib, st = L.lib(), L.stream(gpu_device)
    desc, _ = ops.convert_features([one], [feat], 1, 1, H, W)
    out = torch.full((H * W,), 7.0, device=gpu_device)
    assert lib.p4c_pack_convert(L.ptr(desc), L.ptr(out), 1, 0, 1, 1, H, W, 145, st) == L.ERR_INVALID
    assert lib.p4c_pack_convert(L.ptr(desc), L.ptr(out), 1, 0, 1 << 15, 1 << 4, 64, 64, 1, st) == L.ERR_INVALID
    assert lib.p4c_pack_convert(L.ptr(desc), L.ptr(out), 7, 0, 1, 1, H, W, 1, st) == L.ERR_INVALID
    assert lib.p4c_pack_convert(L.ptr(desc), L.ptr(out), 1, 1, 1, 1, W, H + 1, 1, st) == L.ERR_INVALID     # vec with W = 9
    assert lib.p4c_pack_convert(None, L.ptr(out), 1, 0, 1, 1, H, W, 1, st) == L.ERR_INVALID
    torch.cuda.synchronize(gpu_device)
    assert bool((out == 7.0).all())


def test_typed_titan_reader_equals_the_host_statement(gpu_device, tmp_path):
    """``diskio.load_titan_typed_batch`` on the device (pinned typed planes, one copy, p4c_pack_convert) against the same call on the host"""
    import datetime as dt

    from py4cast_amd import base, diskio
    from py4cast_amd.namedtensor import NamedTensor

    rng = np.random.default_rng(9)
    params = [("aro_t2m", 2, "heightAboveGround"), ("aro_t", 850, "isobaricInhPa"), ("aro_t", 500, "isobaricInhPa")]
    dates = [[dt.datetime(2023, 3, 1, 6 * b + t) for t in range(3)] for b in range(2)]
    stats = base.Stats({n: {"mean": torch.tensor(270.0 + i), "std": torch.tensor(6.0 + i)} for i, n in enumerate(("aro_t2m_2m", "aro_t_850hpa", "aro_t_500hpa"))})
    for dtype, (H, W) in (("<f8", (5, 7)), ("<f2", (16, 24)), ("<u2", (33, 47))):
        root = tmp_path / dtype[1:]
        for (n, lv, lt) in params:
            for ds in dates:
                for d in ds:
                    path = diskio.titan_plane_path(root, n, lv, lt, d)
                    path.parent.mkdir(parents=True, exist_ok=True)
                    np.save(path, make_planes(dtype, (H, W), rng))
        forcing = NamedTensor(torch.zeros(2, 2, H, W, 5), ["batch", "timestep", "lat", "lon", "features"], [f"g{i}" for i in range(5)])
        host = diskio.load_titan_typed_batch(root, params, dates, stats, 1, forcing, host=True)
        dev = diskio.load_titan_typed_batch(root, params, dates, stats, 1, forcing, device=gpu_device)
        # one reader used again while the consumer's stream is busy: each call returns its own planes (the pinned buffer is refilled
        # only after the copy that last read it)
        shape, dt_ = (H, W), np.dtype(dtype)
        reader = diskio.TypedNpyPlaneReader(shape, dt_, 3, 2, 3, device=gpu_device)
        later = [[d + dt.timedelta(days=1) for d in ds] for ds in dates]
        for (n, lv, lt) in params:
            for ds in later:
                for d in ds:
                    path = diskio.titan_plane_path(root, n, lv, lt, d)
                    path.parent.mkdir(parents=True, exist_ok=True)
                    np.save(path, make_planes(dtype, (H, W), rng))
        first = diskio.load_titan_typed_batch(root, params, dates, stats, 1, forcing, reader=reader)
        second = diskio.load_titan_typed_batch(root, params, later, stats, 1, forcing, reader=reader)
        R.assert_bit_equal(first.outputs.tensor.cpu().numpy(), host.outputs.tensor.numpy(), dtype + " reader reused, first")
        R.assert_bit_equal(second.outputs.tensor.cpu().numpy(),
                           diskio.load_titan_typed_batch(root, params, later, stats, 1, forcing, host=True).outputs.tensor.numpy(), dtype + " second")
        assert dev.inputs.tensor.device == gpu_device and dev.outputs.tensor.shape == (2, 2, H, W, 3)
        R.assert_bit_equal(dev.inputs.tensor.cpu().numpy(), host.inputs.tensor.numpy(), dtype)
        R.assert_bit_equal(dev.outputs.tensor.cpu().numpy(), host.outputs.tensor.numpy(), dtype)
