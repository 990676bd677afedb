"""
The arithmetic of ``p4c_pack_convert`` on the host: the numpy restatement the GPU tests compare the kernel with
(tests/pack_convert_reference.py) against the reference's float64 formula on the rainfall fixture, within the bound of four
rounded fp32 steps; against the plain standardisation when no transform is set; and against the package's own host statement
(``datapipe.pack_typed_host``, what a loader on the CPU device returns).
"""
import numpy as np
import pytest
import torch

import datasets_fixtures as DF
import pack_convert_reference as R

MEAN, STD = 0.7, 2.3          # the fixture's statistics of "precip"


def rainfall_planes():
    arrays, _ = DF.golden("rainfall")
    planes = np.stack([a for k, a in sorted(arrays.items()) if k.startswith("file::")])
    assert planes.dtype == np.int16 and (planes < 0).any() and planes.max() == 32767 and planes.min() == -32768
    return planes[None]          # (1, T, 16, 16)


def test_restatement_against_the_float64_formula_on_the_rainfall_fixture():
    x = rainfall_planes()
    got = R.pack_convert_reference([x], [dict(floor=0.0, div=100.0, mul=12.0, flip=True, mean=MEAN, std=STD)])[..., 0].astype(np.float64)
    # rainfall.py:150-155 then base.py:448-452, float64 throughout; the statistics are the fp32 values the files hold
    mean, std = float(np.float32(MEAN)), float(np.float32(STD))
    v = (np.where(x < 0, 0, x) / 100 * 12)[..., ::-1, :]
    want = (v - mean) / std
    # four rounded fp32 steps (/ 100, * 12, - mean, / std; the conversion of an int16 and the floor are exact), each within
    # 2^-24 relative of its own result, none of which exceeds |v'| + |mean| before the division by |std|
    bound = 4 * 2.0 ** -24 * (np.abs(v) + abs(mean)) / abs(std)
    err = np.abs(got - want)
    print(f"worst error / bound: {float((err / bound).max()):.3f} over {err.size} values")
    assert (err <= bound).all()
    assert (got[v == 0] == np.float32(np.float32(0 - np.float32(MEAN)) / np.float32(STD))).all() and (x < 0).sum() > 100


@pytest.mark.parametrize("dtype", R.NP_DTYPES)
def test_without_transform_it_is_the_plain_standardisation(dtype):
    rng = np.random.default_rng(5)
    dt = np.dtype(dtype)
    x = (rng.standard_normal((2, 3, 5, 7)) * 50).astype(dt) if dt.kind == "f" else rng.integers(0, 200, (2, 3, 5, 7)).astype(dt)
    mean, std = np.float32(1.25), np.float32(0.3)
    got = R.pack_convert_reference([x], [dict(mean=mean, std=std)])
    with np.errstate(all="ignore"):
        want = (x.astype(np.float32) - mean) / std
    assert want.dtype == np.float32
    R.assert_bit_equal(got[..., 0], want, dtype)
    # a div / mul of exactly 1 and no floor are skipped, so they change nothing either
    R.assert_bit_equal(R.pack_convert_reference([x], [dict(floor=None, div=1.0, mul=1.0, flip=False, mean=mean, std=std)]), got, dtype)


def test_the_packages_host_statement_is_the_same_arithmetic():
    from py4cast_amd import datapipe

    rng = np.random.default_rng(6)
    planes, feats, trs = [], [], []
    for i, dtype in enumerate(R.NP_DTYPES):
        dt = np.dtype(dtype)
        x = (rng.standard_normal((2, 2, 6, 5)) * 300).astype(dt) if dt.kind == "f" else \
            rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, (2, 2, 6, 5), endpoint=True).astype(dt)
        if dt.kind == "f":
            x[0, 0, 0, :2] = [np.nan, -1.0]
        flip, floor, div, mul = bool(i & 1), (0.0 if i & 2 else None), (100.0 if i & 4 else 1.0), (12.0 if i & 4 else 1.0)
        planes.append(x)
        feats.append(dict(floor=floor, div=div, mul=mul, flip=flip, mean=0.1 * i, std=1.0 + 0.2 * i))
        trs.append(datapipe.PlaneTransform(floor, div, mul, flip))
    want = R.pack_convert_reference(planes, feats)
    got = datapipe.pack_typed_host(planes, trs, [f["mean"] for f in feats], [f["std"] for f in feats])
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32
    R.assert_bit_equal(got.numpy(), want, "pack_typed_host")
    # a NaN stays a NaN under the floor (one per float plane, wherever the flip puts it), the -1 beside it is floored
    assert (np.isnan(want[..., 4:]).sum(axis=(0, 1, 2, 3)) == 1).all() and not np.isnan(want[..., :4]).any()
    assert datapipe.RAINFALL_TRANSFORM == datapipe.PlaneTransform(0.0, 100.0, 12.0, True)


def test_load_typed_batch_on_the_host():
    from py4cast_amd import base, datapipe
    from py4cast_amd.namedtensor import NamedTensor

    x = rainfall_planes()[:, :5]
    stats = base.Stats({"precip": {"mean": torch.tensor(MEAN), "std": torch.tensor(STD)}})
    forcing = NamedTensor(torch.zeros(1, 3, 16, 16, 5), datapipe.DIMS.copy(), [f"g{i}" for i in range(5)])
    planes = torch.from_numpy(x[None].copy())
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # planes on the host are refused unless the host statement is asked for
        datapipe.load_typed_batch(planes, ["precip"], datapipe.RAINFALL_TRANSFORM, forcing, stats, 2)
    batch = datapipe.load_typed_batch(planes, ["precip"], datapipe.RAINFALL_TRANSFORM, forcing, stats, 2, host=True)
    want = R.pack_convert_reference([x], [dict(floor=0.0, div=100.0, mul=12.0, flip=True, mean=MEAN, std=STD)])
    assert batch.inputs.tensor.shape == (1, 2, 16, 16, 1) and batch.outputs.tensor.shape == (1, 3, 16, 16, 1)
    assert batch.inputs.feature_names == batch.outputs.feature_names == ["precip"] and batch.forcing is forcing
    R.assert_bit_equal(torch.cat([batch.inputs.tensor, batch.outputs.tensor], 1).numpy(), want, "load_typed_batch")


def test_launch_arithmetic_restated():
    assert [R.rows_per_pass(F) for F in (1, 2, 3, 8, 9, 16, 21, 144)] == [2048, 2048, 1280, 512, 256, 256, 256, 256]
    side = R.two_trip_side(9, 1, 256)
    assert R.trips(side * side, 9, 256) == 2 and R.trips((side - 1) ** 2, 9, 256) == 1
    assert R.two_trip_side(1, 1, 256, multiple_of=16) % 16 == 0


def test_typed_titan_reader_on_the_host(tmp_path):
    """``diskio.load_titan_typed_batch``: float64 and int16 planes reach the pack in their own dtype; the result is the arithmetic above"""
    import datetime as dt

    from py4cast_amd import base, diskio
    from py4cast_amd.namedtensor import NamedTensor

    rng = np.random.default_rng(8)
    params = [("aro_t2m", 2, "heightAboveGround"), ("aro_t", 850, "isobaricInhPa")]
    dates = [[dt.datetime(2023, 3, 1, 6 * b + t) for t in range(3)] for b in range(2)]
    stats = base.Stats({"aro_t2m_2m": {"mean": torch.tensor(280.0), "std": torch.tensor(8.0)},
                        "aro_t_850hpa": {"mean": torch.tensor(270.0), "std": torch.tensor(6.0)}})
    forcing = NamedTensor(torch.zeros(2, 2, 5, 7, 5), ["batch", "timestep", "lat", "lon", "features"], [f"g{i}" for i in range(5)])
    for dtype in ("<f8", "<i2"):
        root = tmp_path / dtype[1:]
        planes = {}
        for (n, lv, lt) in params:
            for b in range(2):
                for t in range(3):
                    path = diskio.titan_plane_path(root, n, lv, lt, dates[b][t])
                    path.parent.mkdir(parents=True, exist_ok=True)
                    planes[n, b, t] = (rng.standard_normal((5, 7)) * 7 + 275).astype(dtype)
                    np.save(path, planes[n, b, t])
        batch = diskio.load_titan_typed_batch(root, params, dates, stats, 1, forcing, host=True)
        x = [np.stack([np.stack([planes[n, b, t] for t in range(3)]) for b in range(2)]) for (n, _, _) in params]
        want = R.pack_convert_reference(x, [dict(mean=280.0, std=8.0), dict(mean=270.0, std=6.0)])
        assert batch.inputs.feature_names == ["aro_t2m_2m", "aro_t_850hpa"] and batch.inputs.tensor.shape == (2, 1, 5, 7, 2)
        R.assert_bit_equal(torch.cat([batch.inputs.tensor, batch.outputs.tensor], 1).numpy(), want, dtype)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diskio.load_titan_typed_batch(root, params, dates, stats, 1, forcing)
    with pytest.raises(ValueError, match="expected"):
        diskio.TypedNpyPlaneReader((5, 7), "<f4", 2, 2, 3).read(
            [[[diskio.titan_plane_path(root, n, lv, lt, d) for d in ds] for ds in dates] for (n, lv, lt) in params])
