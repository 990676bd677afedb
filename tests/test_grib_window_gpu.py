"""
``ops.grib_window_pack`` / ``datapipe.load_window_batch`` (csrc/grib_window.hip) on the GPU, bit for bit (``torch.equal``) against its
numpy statement ``grib2.unpack_window`` and against the two-launch route it replaces: ``GribPlaneReader.read`` (``p4c_grib_unpack``,
whole streams) followed by ``datapipe.load_native_batch`` with the identity plan (``p4c_regrid_pack``).  Every call runs twice, with
the bytes between and after the slices 0x00 and then 0xFF: equal outputs say that nothing outside a slice is read and that two calls
give the same bits.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_unpack_cases as cases  # noqa: E402
import grib_window_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu
NJ, NI = wc.NJ, wc.NI
SUB = (4, 23, 6, 29)            # a window of 19 x 23 = 437 pixels: no multiple of 256, workgroups straddle (b, t) planes


def _case(tmp_path, device, specs, B, T, grid=(NJ, NI), sub=SUB, seed=0, standardize=True, scan=None, two_launch=True):
    """-> (the window batch, its numpy statement, the two-launch batch or None)"""
    from py4cast_amd import datapipe, grib2, regrid
    from py4cast_amd.diskio import GribPlaneReader

    g = np.random.default_rng(seed)
    F = len(specs)
    nj, ni = grid
    msgs = wc.messages(g, B, T, specs, nj=nj, ni=ni, scan=scan)
    fields = [[[grib2.field_of(m) for m in per_b] for per_b in per_f] for per_f in msgs]
    names = [f"f{f}" for f in range(F)]
    stats = wc.Stats({n: (float(np.float32(g.normal() * 5)), float(np.float32(0.5 + g.random()))) for n in names})
    plan = regrid.RegridPlan(grid, grid, subdomain=sub)
    rows = datapipe.window_rows(plan)
    got = []
    for fill in (0x00, 0xFF):
        buf, places = wc.slices_buffer(fields, rows, fill)
        table = datapipe.window_table(fields, places, names, plan)
        batch = datapipe.load_window_batch(torch.from_numpy(buf).to(device), table, names, None, stats, 1, standardize)
        got.append(torch.cat([batch.inputs.tensor, batch.outputs.tensor], dim=1))
        assert batch.inputs.feature_names == batch.outputs.feature_names == names and batch.inputs.tensor.shape[1] == 1
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)), "the bytes around the slices changed the output"
    H, W = plan.out_shape
    assert got[0].shape == (B, T, H, W, F) and got[0].dtype == torch.float32 and got[0].is_contiguous()
    want = np.empty((B, T, H, W, F), dtype=np.float32)
    for f in range(F):
        mean, std = (stats.table[names[f]] if standardize else (0.0, 1.0))
        for b in range(B):
            for t in range(T):
                # the plan flips the north-first plane: output row y is row rows[1] - 1 - y
                want[b, t, :, :, f] = grib2.unpack_window(fields[f][b][t], (*rows, sub[2], sub[3]), mean, std)[::-1]
    ref = None
    if two_launch:
        planes, _, _ = GribPlaneReader(device=device).read(wc.write_files(str(tmp_path), msgs))
        old = datapipe.load_native_batch([(planes, names, plan)], names, None, stats, 1, standardize)
        ref = torch.cat([old.inputs.tensor, old.outputs.tensor], dim=1)
    return got[0], torch.from_numpy(want), ref


@pytest.mark.parametrize("south_to_north", [False, True])
@pytest.mark.parametrize("nbits", wc.NBITS)
def test_every_width_and_scale_in_both_scanning_directions(nbits, south_to_north, gpu_device, tmp_path):
    """B x T = 2 x 3, F = 3: D = -2, 0, 3 with a negative E, one width per call"""
    g = np.random.default_rng(nbits)
    specs = [(nbits, float(np.float32(g.normal() * 30)), -3, D) for D in wc.DS]
    got, want, ref = _case(tmp_path, gpu_device, specs, 2, 3, seed=nbits, scan=lambda f, b, t: south_to_north)
    assert torch.equal(got.cpu(), want) and torch.equal(got, ref)
    assert bool(torch.isfinite(got).all()) and (nbits == 0 or float(got.std()) > 0)


@pytest.mark.parametrize("F", [1, 3, 21])
def test_fields_of_mixed_width_reference_and_scales_in_one_call(F, gpu_device, tmp_path):
    """every feature its own nbits, R, E, D; the scanning direction alternates with b + t"""
    g = np.random.default_rng(40 + F)
    specs = [wc.spec_of(f + (4 if F == 1 else 0), g) for f in range(F)]
    got, want, ref = _case(tmp_path, gpu_device, specs, 2, 3, seed=F)
    assert torch.equal(got.cpu(), want) and torch.equal(got, ref)


def test_sixteen_bits_on_rows_of_a_multiple_of_eight(gpu_device, tmp_path):
    """40 x 64 points, a window of 30 x 56 at F = 5: more than 2 x 256 rows per plane, W a multiple of 8, 16 bits throughout"""
    g = np.random.default_rng(77)
    specs = [(16, float(np.float32(g.normal() * 30)), (-4, -1, 0, 1, -7)[f], wc.DS[f % 3]) for f in range(5)]
    got, want, ref = _case(tmp_path, gpu_device, specs, 2, 2, grid=(40, 64), sub=(5, 35, 8, 64), seed=77)
    assert got.shape == (2, 2, 30, 56, 5) and torch.equal(got.cpu(), want) and torch.equal(got, ref)


def test_a_window_smaller_than_a_workgroup(gpu_device, tmp_path):
    """a window of 5 x 7 = 35 pixels at B x T = 2 x 3: the one workgroup of 256 rows walks over all six (b, t) planes, every lane finds
    its own plane and descriptor, and the rows past the end store nothing"""
    g = np.random.default_rng(5)
    specs = [wc.spec_of(f, g) for f in (1, 4, 6)]
    got, want, ref = _case(tmp_path, gpu_device, specs, 2, 3, sub=(4, 9, 6, 13), seed=5)
    assert got.shape == (2, 3, 5, 7, 3) and torch.equal(got.cpu(), want) and torch.equal(got, ref)


def test_standardize_off_returns_the_decoded_values(gpu_device, tmp_path):
    g = np.random.default_rng(8)
    specs = [wc.spec_of(f, g) for f in (2, 3, 4, 7)]
    got, want, ref = _case(tmp_path, gpu_device, specs, 1, 2, seed=8, standardize=False)
    assert torch.equal(got.cpu(), want) and torch.equal(got, ref)
    from py4cast_amd import grib2

    msgs = wc.messages(np.random.default_rng(8), 1, 2, specs)            # the same messages: the values ``grib2.decode`` gives
    plane = wc.expected_window(msgs[2][0][1], (0, NJ, 0, NI))
    assert cases.same_bits(got[0, 1, :, :, 2].cpu().numpy(), plane[::-1][SUB[0]:SUB[1], SUB[2]:SUB[3]])
    assert grib2.field_of(msgs[2][0][1]).nbits == 16


def test_refusals_before_any_launch(gpu_device):
    from py4cast_amd import _lib, datapipe, grib2, ops, regrid

    g = np.random.default_rng(2)
    field = grib2.field_of(cases.random_message(g, NI, NJ, 12, 1.0, -2, 1))
    plan = regrid.RegridPlan((NJ, NI), (NJ, NI), subdomain=SUB)
    rows = datapipe.window_rows(plan)
    buf, places = wc.slices_buffer([[[field]]], rows, 0xEE)
    dev = torch.from_numpy(buf).to(gpu_device)
    good = datapipe.window_table([[[field]]], places, ["a"], plan).fields.reshape(-1)
    H, W = plan.out_shape
    ops.grib_window_pack(dev, good, 1, 1, H, W, 1)                        # the record itself is accepted
    with pytest.raises(_lib.P4CError, match="145 features"):
        ops.grib_window_pack(dev, np.repeat(good, 145), 1, 1, H, W, 145)
    bad = good.copy()
    bad["slice_off"] += 2
    with pytest.raises(_lib.P4CError, match="multiples of 4"):
        ops.grib_window_pack(dev, bad, 1, 1, H, W, 1)
    bad = good.copy()
    bad["bitmap_off"] = 0
    with pytest.raises(_lib.P4CError, match="bitmap"):
        ops.grib_window_pack(dev, bad, 1, 1, H, W, 1)
    bad = good.copy()
    bad["slice_len"] = 100                                                # the window's last rows would lie outside the slice
    with pytest.raises(_lib.P4CError, match="leave the slice"):
        ops.grib_window_pack(dev, bad, 1, 1, H, W, 1)
    bad = good.copy()
    bad["slice_len"] = buf.size                                           # a slice that leaves the buffer
    with pytest.raises(_lib.P4CError, match="leaves the"):
        ops.grib_window_pack(dev, bad, 1, 1, H, W, 1)
    masked = grib2.field_of(cases.random_message(g, NI, NJ, 12, 1.0, -2, 1, present=g.random(NI * NJ) < 0.9))
    with pytest.raises(ValueError, match="not a simple-packed field without bitmap"):
        datapipe.window_table([[[masked]]], places, ["a"], plan)
    torch.cuda.synchronize()
