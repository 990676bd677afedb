"""
numpy restatement of ``p4c_pack_convert`` (include/py4cast_hip.h), the reference of tests/test_pack_convert_*.py, and the
kernel's launch arithmetic restated for the tests that size a second loop trip.

Every step is a numpy float32 operation, hence rounded to nearest even once, exactly as the kernel's fp32 instructions are:
``astype(float32)``, the floor by ``np.where`` (a NaN compares false and stays), ``/ div``, ``* mul`` (a factor of exactly 1 is
skipped), ``- mean``, ``/ std``.
"""
import numpy as np

F4 = np.float32
NP_DTYPES = ("u1", "<i2", "<u2", "<i4", "<f2", "<f4", "<f8")

# the launch arithmetic of csrc/pack_convert.hip
BASE_ROWS = 256
BLOCKS_PER_CU = 8


def rows_per_pass(F):
    return BASE_ROWS * min(8, max(16 // F, 1))


def passes(rows, F):
    return -(-rows // rows_per_pass(F))


def trips(rows, F, cus):
    """loop trips of the busiest workgroup"""
    return -(-passes(rows, F) // min(passes(rows, F), cus * BLOCKS_PER_CU))


def two_trip_side(F, BT, cus, multiple_of=1):
    """smallest H = W (a multiple of ``multiple_of``) at which BT planes of H x W send a workgroup through a second pass"""
    side = max(int((cus * BLOCKS_PER_CU * rows_per_pass(F) / BT) ** 0.5) // multiple_of * multiple_of, multiple_of)
    while trips(BT * side * side, F, cus) < 2:
        side += multiple_of
    return side


def transform_plane(x, floor=None, div=1.0, mul=1.0, flip=False):
    """(..., H, W) of any dtype -> float32, the transform steps before the standardisation"""
    with np.errstate(all="ignore"):
        v = np.asarray(x).astype(F4)
        if floor is not None:
            v = np.where(v < F4(floor), F4(floor), v)
        if F4(div) != F4(1):
            v = v / F4(div)
        if F4(mul) != F4(1):
            v = v * F4(mul)
    if flip:
        v = v[..., ::-1, :]
    return np.ascontiguousarray(v, dtype=F4)


def pack_convert_reference(planes, feats):
    """planes: per output feature a (B, T, H, W) array in its file dtype (channel order); feats: per feature a dict with the keys
    floor (None: no floor), div, mul, flip, mean, std -> (B, T, H, W, F) float32"""
    cols = []
    with np.errstate(all="ignore"):
        for x, d in zip(planes, feats):
            v = transform_plane(x, d.get("floor"), d.get("div", 1.0), d.get("mul", 1.0), d.get("flip", False))
            cols.append((v - F4(d.get("mean", 0.0))) / F4(d.get("std", 1.0)))
    out = np.stack(cols, axis=-1)
    assert out.dtype == F4
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=F4).view(np.uint32)


def assert_bit_equal(got, want, what=""):
    """bit for bit, except that any NaN equals any NaN (the payload of a NaN is not part of the definition)"""
    got, want = np.asarray(got, dtype=F4), np.asarray(want, dtype=F4)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), f"{what}: NaN positions differ ({nan_g.sum()} vs {nan_w.sum()})"
    bad = (bits(got) != bits(want)) & ~nan_w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}: " \
                          f"{got[bad][0]!r} vs {want[bad][0]!r}"
