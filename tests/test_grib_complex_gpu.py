"""
``ops.grib_unpack_complex`` (csrc/grib_complex.hip) on the GPU against the integers handed to the encoder of
tests/grib_complex_cases.py: every plane bit for bit, every call twice with identical bits, the planes inside sentinel guards with
gaps, the status words, and the refusals that launch nothing.  Sizes are relative to the launch constants the library reports:
T = values per tile, C = groups per chunk, CAP = the most workgroups of a launch.
"""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_complex_cases as cc  # noqa: E402
import test_grib_complex_cpu as host  # noqa: E402

pytestmark = pytest.mark.gpu


def constants():
    from py4cast_amd import _lib

    lib = _lib.lib()
    return lib.p4c_grib_complex_tile(), lib.p4c_grib_complex_chunk(), lib.p4c_grib_complex_max_blocks()


def run(device, messages, wants, flips=None, gap=8, lead=12, tail=5, statuses=None, fields=None):
    """decode the messages in ONE call, twice, and compare the whole output buffer -- guards, gaps and padding included -- with the
    expected planes bit for bit, and the status words"""
    from py4cast_amd import grib2, ops

    fields = [grib2.complex_field_of(m) for m in messages] if fields is None else fields
    data, table, floats = cc.layout(fields, flips=flips, gap=gap, lead=lead, tail=tail)
    want = cc.expected_buffer(table, wants, floats)
    dev = torch.from_numpy(data).to(device)
    seen = []
    for _ in range(2):
        out = torch.full((floats,), float(cc.SENTINEL), dtype=torch.float32, device=device)
        status = torch.full((len(fields),), -7, dtype=torch.int32, device=device)
        got, st = ops.grib_unpack_complex(dev, table, out=out, status=status)
        torch.cuda.synchronize()
        assert got is out and st is status
        seen.append((out.cpu().numpy(), status.cpu().numpy()))
    assert np.array_equal(seen[0][0].view(np.int32), seen[1][0].view(np.int32)) and np.array_equal(seen[0][1], seen[1][1])
    planes, st = seen[0]
    if statuses is None:
        assert not st.any(), st
    else:
        assert [int(s) & bit == bit and (bit != 0 or int(s) == 0) for s, bit in zip(st, statuses)] == [True] * len(fields), st
    assert cc.same_bits(planes, want), np.flatnonzero(~((planes.view(np.int32) == want.view(np.int32)) | (np.isnan(planes) & np.isnan(want))))[:8]
    return planes, st


def bitmap_of(kind, g, ni, nj, T):
    n = ni * nj
    if kind == "none":
        return None
    if kind == "random":
        return g.random(n) < 0.6
    if kind == "window":
        return cc.window_present(ni, nj, min(5, nj - 1), max(nj - 9, min(5, nj - 1)), 0 if ni < 8 else 3, ni - 1 if ni < 8 else ni - 6)
    assert kind == "last_tile"
    present = np.zeros(n, dtype=bool)
    present[(n - 1) // T * T:] = True
    return present


# 2T + 37 is prime: 2T + 37 points as rows of one point, and 2T + 62 points as 66 rows of 63
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("kind", ["none", "random", "window", "last_tile"])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_every_order_bitmap_and_direction(order, kind, flip, gpu_device):
    T, _, _ = constants()
    assert 2 * T + 62 == 66 * 63
    g = np.random.default_rng(100 + 10 * order + len(kind))
    messages, wants = [], []
    for ni, nj in ((1, 2 * T + 37), (63, 66)):
        present = bitmap_of(kind, g, ni, nj, T)
        n = ni * nj if present is None else int(present.sum())
        f = cc.smooth_field(g, n, offset=4000 if order == 0 else -300)
        messages.append(cc.message(ni, nj, f, order, cc.random_bounds(g, n), 250.0, -1, 1, present=present, south_to_north=flip))
        wants.append(cc.expected_plane(f, ni, nj, 250.0, -1, 1, present=present, flip=flip))
    run(gpu_device, messages, wants, flips=[flip, flip])


def test_the_worked_example_on_the_device(gpu_device):
    planes, _ = run(gpu_device, [host.example_message()], [cc.expected_plane(host.EXAMPLE_F, 5, 2, 250.0, -1, 1)], gap=0, lead=0)
    assert [int(v) for v in planes[cc.GUARD:cc.GUARD + 10].view(np.uint32)] == host.EXAMPLE_BITS


@pytest.mark.parametrize("name", list(host.HOST_CASES))
def test_the_cases_of_the_host(name, gpu_device):
    ni, nj, f, order, bounds, R, E, D, present, s2n, params = host.HOST_CASES[name]
    msg = cc.message(ni, nj, f, order, bounds, R, E, D, present=present, south_to_north=s2n, **params)
    run(gpu_device, [msg], [cc.expected_plane(f, ni, nj, R, E, D, present=present, flip=s2n)], flips=[s2n])


@pytest.mark.parametrize("order", [0, 1, 2])
def test_groups_that_straddle_the_tile_boundaries(order, gpu_device):
    T, _, _ = constants()
    g = np.random.default_rng(7)
    ni, nj = 63, 66
    f = cc.smooth_field(g, ni * nj, offset=4000 if order == 0 else 0)
    bounds = [0, 3, T - 5, T + 9, 2 * T - 1, 2 * T + 1, 2 * T + 40]
    msg = cc.message(ni, nj, f, order, bounds, 1.0, -3, 2, l_bits=12)
    run(gpu_device, [msg], [cc.expected_plane(f, ni, nj, 1.0, -3, 2)])


@pytest.mark.parametrize("width", [0, 7])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_one_group_of_three_tiles_and_five_values(order, width, gpu_device):
    T, _, _ = constants()
    ni, nj = 143, 43
    assert ni * nj == 3 * T + 5
    g = np.random.default_rng(9)
    X = np.full(ni * nj, 77, dtype=np.int64) if width == 0 else 1000 + g.integers(0, 128, size=ni * nj)
    X[:2] = X[2]
    if width:
        X[5], X[6] = 1000, 1127
    f = X if order == 0 else np.cumsum(X - 1050) if order == 1 else np.cumsum(np.cumsum(X - 1063))
    msg = cc.message(ni, nj, f, order, [0], 10.0, 0, 0, widths=[width], nbytes=4, l_bits=0)
    run(gpu_device, [msg], [cc.expected_plane(f, ni, nj, 10.0, 0, 0)])


def test_width_32_behind_references_of_32_bits(gpu_device):
    g = np.random.default_rng(10)
    ni, nj = 25, 12
    top = 2 ** 32 - 1
    f = g.integers(0, top + 1, size=ni * nj, dtype=np.int64)
    bounds = cc.random_bounds(g, ni * nj, 2, 12)
    for b in bounds[:-1]:                                     # every group but the last spans 32 bits: a value of 0 and one of 2^32 - 1 ...
        f[b], f[b + 1] = 0, top
    f[bounds[3]:bounds[4]] = top                              # ... but one constant at the largest reference, and one whose sums reach 2^33 - 2
    f = f.astype(object)
    f[bounds[5]:bounds[6]] += top                             # X from 2^32 - 1 to 2^33 - 2
    msg = cc.message(ni, nj, f, 0, bounds, 0.0, -7, 0, ref_bits=32, w_bits=6)
    want = cc.expected_plane(np.array([int(v) for v in f], dtype=np.int64), ni, nj, 0.0, -7, 0)
    run(gpu_device, [msg], [want])
    wide, wide_bounds = cc.wide_field()
    run(gpu_device, [cc.message(6, 3, wide, 0, wide_bounds, 0.0, 0, 0, ref_bits=32, w_bits=6)], [cc.expected_plane(wide, 6, 3, 0.0, 0, 0)])


@pytest.mark.parametrize("groups", ["C+1", "2C+3"])
def test_groups_past_one_chunk(groups, gpu_device):
    """a chunk's base is summed over the chunks before it, and the bisection over the groups' first values crosses chunks"""
    _, C, _ = constants()
    ng = C + 1 if groups == "C+1" else 2 * C + 3
    g = np.random.default_rng(11)
    lengths = g.integers(1, 4, size=ng)
    ni = 37
    lengths[-1] += -int(lengths.sum()) % ni                   # whole rows
    n = int(lengths.sum())
    bounds = list(np.cumsum(lengths) - lengths)
    present = None
    for order, flip in ((2, False), (0, True), (1, True)):
        f = cc.smooth_field(g, n, offset=4000 if order == 0 else -5, noise=40)
        msg = cc.message(ni, n // ni, f, order, bounds, 3.0, -1, 0, present=present, south_to_north=flip, l_bits=6)
        run(gpu_device, [msg], [cc.expected_plane(f, ni, n // ni, 3.0, -1, 0, flip=flip)], flips=[flip])


def test_the_wrap_around_field_over_three_tiles(gpu_device):
    T, _, _ = constants()
    ni, nj = 96, 3 * T // 96
    assert ni * nj == 3 * T
    g = np.random.default_rng(12)
    f = cc.wrap_field(g, 3 * T)
    d = f[2:] - 2 * f[1:-1] + f[:-2]
    assert np.abs(np.cumsum(d)).max() > 2 ** 32
    msg = cc.message(ni, nj, f, 2, cc.random_bounds(g, 3 * T), 0.0, -20, 0, nbytes=4, ref_bits=32)
    run(gpu_device, [msg], [cc.expected_plane(f, ni, nj, 0.0, -20, 0)])


def test_counts_of_0_1_and_2(gpu_device):
    nothing = cc.message(9, 5, [], 1, [], 1.0, 0, 0, present=np.zeros(45, dtype=bool))
    nothing52 = cc.message(9, 5, [], 0, [], 1.0, 0, 0, present=np.zeros(45, dtype=bool))
    one = cc.message(1, 1, [-77], 1, [0], 2.0, 0, 0)
    one2 = cc.message(1, 1, [-77], 2, [0], 2.0, 0, 0)
    two = cc.message(2, 1, [-77, 12], 2, [0], 2.0, 0, 0)
    two_groups = cc.message(1, 2, [-77, 12], 2, [0, 1], 2.0, 0, 0, south_to_north=True)
    wants = [np.full((5, 9), np.nan, dtype=np.float32)] * 2 + [cc.expected_plane([-77], 1, 1, 2.0, 0, 0)] * 2 + \
        [cc.expected_plane([-77, 12], 2, 1, 2.0, 0, 0), cc.expected_plane([-77, 12], 1, 2, 2.0, 0, 0, flip=True)]
    run(gpu_device, [nothing, nothing52, one, one2, two, two_groups], wants, flips=[False] * 5 + [True])


def test_three_fields_of_different_sizes_orders_and_templates(gpu_device):
    T, _, _ = constants()
    g = np.random.default_rng(13)
    messages, wants, flips = [], [], []
    for (ni, nj), order, masked, flip in (((53, 17), 2, True, True), ((2 * T // 64 + 1, 64), 0, False, False), ((7, 3), 1, False, True)):
        present = (g.random(ni * nj) < 0.5) if masked else None
        n = ni * nj if present is None else int(present.sum())
        f = cc.smooth_field(g, n, offset=4000 if order == 0 else -17)
        messages.append(cc.message(ni, nj, f, order, cc.random_bounds(g, n), -4.0, -2, -1, present=present, south_to_north=flip))
        wants.append(cc.expected_plane(f, ni, nj, -4.0, -2, -1, present=present, flip=flip))
        flips.append(flip)
    run(gpu_device, messages, wants, flips=flips, gap=12, lead=8)


def test_one_tile_and_one_chunk_more_than_the_launch_has_workgroups(gpu_device):
    """CAP + 1 tiny fields, a tile and a chunk each: every workgroup of the tile and of the chunk launches takes two and walks from
    one field into the next"""
    _, _, CAP = constants()
    g = np.random.default_rng(14)
    messages, wants, flips = [], [], []
    present = np.array([1, 0, 1, 1, 0, 1], dtype=bool)
    for i in range(CAP + 1):
        order, masked, flip = i % 3, i % 5 == 0, i % 2 == 1
        n = int(present.sum()) if masked else 6
        f = g.integers(0, 50, size=n) + i
        messages.append(cc.message(3, 2, f, order, [0, 2][:1 + i % 2], 1.0, 0, 0, present=present if masked else None, south_to_north=flip))
        wants.append(cc.expected_plane(f, 3, 2, 1.0, 0, 0, present=present if masked else None, flip=flip))
        flips.append(flip)
    run(gpu_device, messages, wants, flips=flips, gap=4)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", ["lengths", "width", "stream"])
def test_a_status_condition_on_the_middle_field_of_three(kind, masked, gpu_device):
    from py4cast_amd import grib2

    T, _, _ = constants()
    g = np.random.default_rng(15)
    ni, nj = 61, 70                                            # more than a tile of values, with the bitmap too
    present = (g.random(ni * nj) < 0.7) if masked else None
    n = ni * nj if present is None else int(present.sum())
    assert n > T
    bad, bit, _ = cc.malformed(kind, ni=ni, nj=nj, present=present)
    good = []
    for order in (1, 2):
        f = cc.smooth_field(g, n)
        good.append((cc.message(ni, nj, f, order, cc.random_bounds(g, n), 1.5, -2, 1, present=present), cc.expected_plane(f, ni, nj, 1.5, -2, 1, present=present)))
    nan = np.full((nj, ni), np.nan, dtype=np.float32)
    _, st = run(gpu_device, [good[0][0], bad, good[1][0]], [good[0][1], nan, good[1][1]], statuses=[0, bit, 0])
    assert int(st[1]) & bit
    with pytest.raises(grib2.GribError):                      # the host path names the same condition
        grib2.unpack_fields([grib2.complex_field_of(bad)])


def test_every_refusal_before_the_launch_writes_nothing(gpu_device):
    from py4cast_amd import _lib, grib2, ops

    g = np.random.default_rng(16)
    ni, nj = 23, 11
    present = g.random(ni * nj) < 0.5
    plain = grib2.complex_field_of(cc.message(ni, nj, cc.smooth_field(g, ni * nj), 2, cc.random_bounds(g, ni * nj), 1.5, -2, 1))
    masked = grib2.complex_field_of(cc.message(ni, nj, cc.smooth_field(g, int(present.sum())), 1, [0, 9], 1.5, -2, 1, present=present))
    data, table, floats = cc.layout([plain, masked], gap=4)
    dev = torch.from_numpy(data).to(gpu_device)
    out = torch.full((floats,), float(cc.SENTINEL), dtype=torch.float32, device=gpu_device)
    status = torch.full((2,), -7, dtype=torch.int32, device=gpu_device)
    changes = [(0, "ref_bits", 33), (0, "ref_bits", -1), (1, "w_bits", 33), (0, "w_bits", -1), (0, "l_bits", 33), (1, "l_bits", -1),
               (0, "w_ref", 256), (0, "w_ref", -1), (1, "l_inc", 256), (0, "l_inc", -1), (0, "order", 3), (0, "order", -1), (1, "nbytes", 5),
               (0, "nbytes", -1), (0, "ng", 0), (1, "ng", 2 ** 31), (0, "D", 16), (1, "D", -16), (0, "count", ni * nj + 1), (1, "count", -1),
               (0, "count", ni * nj - 1), (0, "stream_off", int(table[0]["stream_off"]) + 2), (1, "stream_off", -4),
               (1, "bitmap_off", int(table[1]["bitmap_off"]) + 1), (1, "bitmap_off", -2), (0, "dst_off", int(table[0]["dst_off"]) + 2),
               (0, "stream_len", plain.table_bits()[3] // 8 - 1), (1, "stream_len", -1), (0, "stream_len", data.size + 1),
               (1, "stream_off", data.size), (1, "bitmap_off", (data.size - 8) // 4 * 4), (0, "ni", 0), (1, "nj", -3), (0, "ng", 2 ** 20)]
    for index, name, value in changes:
        broken = table.copy()
        broken[index][name] = value
        with pytest.raises(_lib.P4CError):
            ops.grib_unpack_complex(dev, broken, out=out, status=status)
    with pytest.raises(_lib.P4CError):
        ops.grib_unpack_complex(dev[1:], table, out=out, status=status)                          # bytes not 4-byte aligned
    with pytest.raises(_lib.P4CError):
        ops.grib_unpack_complex(dev, table, out=out[:floats - cc.GUARD - 8], status=status)       # the last plane does not fit
    with pytest.raises(_lib.P4CError):
        ops.grib_unpack_complex(dev, table, out=out, status=status[:1])
    with pytest.raises(_lib.P4CError):
        ops.grib_unpack_complex(dev, table[:0], out=out, status=status[:0])
    with pytest.raises(_lib.P4CError):
        ops.grib_unpack_complex(dev.cpu(), table, out=out, status=status)
    # chunk0 and tile0 are ops' to fill in: the library itself checks them
    full = ops.grib_ctable(table, dense=False)
    ws = torch.empty(_lib.lib().p4c_grib_unpack_complex_workspace_bytes(8, 8, 1) // 8 + 1, dtype=torch.int64, device=gpu_device)
    for name in ("tile0", "chunk0"):
        broken = full.copy()
        broken[1][name] += 1
        table_dev = torch.from_numpy(broken.view(np.uint8)).to(gpu_device)
        rc = _lib.lib().p4c_grib_unpack_complex(_lib.ptr(dev), dev.numel(), _lib.ptr(table_dev), ctypes.c_void_p(broken.ctypes.data), 2,
                                                _lib.ptr(out), _lib.ptr(status), _lib.ptr(ws), _lib.stream(gpu_device))
        assert rc == _lib.ERR_INVALID and name in _lib.lib().p4c_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == float(cc.SENTINEL)).all()) and status.tolist() == [-7, -7]
    got, st = ops.grib_unpack_complex(dev, table, out=out, status=status)                        # and the table itself is in order
    assert st.tolist() == [0, 0] and struct.pack("<f", float(got[0])) == struct.pack("<f", float(cc.SENTINEL))
