"""
ops.grib_unpack (csrc/grib_unpack.hip) on the GPU.

The expected plane of every field is ``grib2.decode(message)[0].filled(nan).astype(float32)`` and the comparison is BIT FOR BIT, NaNs by
position: every step of the contract is a single rounded IEEE operation, so there is no tolerance and no excluded element
(tests/test_grib_read_cpu.py checks the numpy restatement the same way, tests/test_grib2_cpu.py ``decode`` against exact rationals).
Every call writes into a sentinel-filled buffer with guards around and gaps between the planes, is made twice, and both results must
have the same bits with guards, gaps and padding intact.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_unpack_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
GAP = 8


def _geometry():
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    handle = L.lib()
    tile, cap = handle.p4c_grib_unpack_tile(), handle.p4c_grib_unpack_max_blocks()
    assert (tile, cap) == (ops.GRIB_UNPACK_TILE, ops.GRIB_UNPACK_MAX_BLOCKS) and tile % 32 == 0
    return tile, cap


def _run(fields, flips, dev, table_edit=None, **kw):
    """-> (the whole output buffer as numpy, the table as launched, its number of floats)"""
    from py4cast_amd import ops

    buf, table, floats = cases.layout(fields, flips, gap=GAP, **kw)
    if table_edit is not None:
        table_edit(table)
    bytes_dev = torch.from_numpy(buf).to(dev)
    outs = []
    for _ in range(2):
        out = torch.full((floats,), float(cases.SENTINEL), dtype=torch.float32, device=dev)
        assert ops.grib_unpack(bytes_dev, table, out=out) is out
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32)), "two calls differ"
    return outs[0], ops.grib_table(table, dense=False), floats


def _check(messages, flips, dev, **kw):
    from py4cast_amd import grib2

    fields = [grib2.field_of(m) for m in messages]
    got, table, floats = _run(fields, flips, dev, **kw)
    want = cases.expected_buffer(table, [cases.expected_plane(m, flip) for m, flip in zip(messages, flips)], floats)
    for i, rec in enumerate(table):      # field by field first: a failure names the field
        a, n = int(rec["dst_off"]), int(rec["ni"]) * int(rec["nj"])
        assert cases.same_bits(got[a:a + n], want[a:a + n]), f"field {i}: nbits {rec['nbits']}, bitmap {rec['bitmap_off'] >= 0}, flip {rec['flip_rows']}"
    assert cases.same_bits(got, want), "a guard, a gap or the padding of a plane was written"
    return got, table


def _shape(N, near=100):
    """(ni, nj) with ni * nj == N, ni the divisor of N closest to ``near``"""
    ni = min((d for d in range(1, N + 1) if N % d == 0), key=lambda d: abs(d - near))
    return ni, N // ni


def test_every_width_without_a_bitmap(gpu_device):
    """33 fields, nbits 0 .. 32, a little more than one tile each: a second tile with a short tail, ragged against 8 and 32.  The issue
    asks for tile + 37 points in rows of 37; the tile is no multiple of 37, so the rows are the fewest that give at least that many."""
    tile, _ = _geometry()
    ni = 37
    nj = -(-(tile + 37) // ni)
    N = ni * nj
    assert tile + 37 <= N < tile + 2 * 37 and N % 8 and N % 32
    g = np.random.default_rng(1)
    messages = []
    for nbits in range(33):
        R = float(np.float32((-1.0) ** nbits * (1.25 + 3.7 * nbits)))
        E = (7 * nbits) % 41 - 30                                   # -30 .. 10
        messages.append(cases.random_message(g, ni, nj, nbits, R, E, (0, 2, -1)[nbits % 3]))
    _, table = _check(messages, [False] * 33, gpu_device)
    assert sorted(table["nbits"]) == list(range(33)) and {int(d) for d in table["D"]} == {0, 2, -1}
    assert (table["E"] < 0).any() and (table["E"] > 0).any() and (table["R"] < 0).any() and (table["tile0"] == 2 * np.arange(33)).all()


@pytest.mark.parametrize("nbits", [9, 12, 16])
def test_bitmaps_and_ranks_across_tiles(nbits, gpu_device):
    tile, _ = _geometry()
    N = 3 * tile + 5
    ni, nj = _shape(N)
    assert ni * nj == N and nj > 1
    g = np.random.default_rng(nbits)
    last = np.zeros(N, dtype=bool)
    last[3 * tile:] = g.random(5) < 0.7                             # the only present points lie in the last tile: its 5 points
    last[N - 1] = True
    assert not last[:3 * tile].any()
    bitmaps = {"half": g.random(N) < 0.5, "ones": np.ones(N, dtype=bool), "zeros": np.zeros(N, dtype=bool),
               "window": cases.window_present(ni, nj, 3, nj - 5, 2, ni - 4), "last": last}
    messages, flips = [], []
    for i, (name, present) in enumerate(bitmaps.items()):
        for flip in (False, True):
            messages.append(cases.random_message(g, ni, nj, nbits, -3.5 + i, -4 + i, (2, 0, -1)[i % 3], present=present))
            flips.append(flip)
    _, table = _check(messages, flips, gpu_device)
    assert (table["bitmap_off"] >= 0).all() and set(table["count"]) >= {0, N} and (table["flip_rows"] == [0, 1] * 5).all()


def test_fields_of_three_sizes_in_one_call(gpu_device):
    from py4cast_amd import grib2, ops

    tile, _ = _geometry()
    g = np.random.default_rng(8)
    sizes = [(40, 24), (37, -(-(tile + 37) // 37)), _shape(3 * tile + 5)]
    messages, flips = [], []
    for i, nbits in enumerate((16, 12, 0, 16, 24, 7, 16, 32, 11)):
        ni, nj = sizes[i % 3]
        present = (g.random(ni * nj) < (0.2, 0.5, 0.9)[i % 3]) if i % 2 else None          # with and without bitmap, interleaved
        messages.append(cases.random_message(g, ni, nj, nbits, 2.0 * i - 5.0, i - 6, (0, 2, -1)[i % 3], present=present, south_to_north=bool(i & 2)))
        flips.append(bool(i & 2))
    _, table = _check(messages, flips, gpu_device)
    assert len({(int(r["ni"]), int(r["nj"])) for r in table}) == 3 and (table["bitmap_off"][1::2] >= 0).all() and (table["bitmap_off"][0::2] < 0).all()
    # without `out`: the planes lie densely, in the order of the table
    fields = [grib2.field_of(m) for m in messages]
    buf, table, _ = cases.layout(fields, flips)
    flat = ops.grib_unpack(torch.from_numpy(buf).to(gpu_device), table).cpu().numpy()
    launched = ops.grib_table(table, dense=True)
    at = 0
    for rec, m, flip in zip(launched, messages, flips):
        n = int(rec["ni"]) * int(rec["nj"])
        assert int(rec["dst_off"]) == at and cases.same_bits(flat[at:at + n], cases.expected_plane(m, flip).reshape(-1))
        at += (n + 3) // 4 * 4
    assert flat.size == at


@pytest.mark.parametrize("bitmap", [False, True])
def test_past_one_loop_trip(bitmap, gpu_device):
    """the smallest number of tiles that sends a workgroup through a second trip, from the library's own launch arithmetic: one
    more than the most workgroups of a launch, so that a workgroup takes ceil(tiles / max_blocks) = 2 consecutive tiles.  Many
    one-tile fields between two fields of two tiles: the first one's tiles 0 and 1 belong to one workgroup, which carries the rank
    over from its first trip; the last one's tiles max_blocks - 1 and max_blocks belong to two workgroups, and the second of them
    adds up the count of the tile before its own.  In between a workgroup changes field in its second trip."""
    tile, cap = _geometry()
    g = np.random.default_rng(21 + bitmap)
    small, (ni, nj) = (7, 3), (37, -(-(tile + 37) // 37))
    big = lambda nbits: cases.random_message(g, ni, nj, nbits, -7.0, -1, 2, present=(g.random(ni * nj) < 0.5) if bitmap else None)  # noqa: E731
    messages = [big(13)]
    for i in range(cap - 3):
        present = (g.random(21) < 0.6) if bitmap else None
        messages.append(cases.random_message(g, *small, (16, 11, 5)[i % 3], 0.5 * (i % 9), -2, (0, 2, -1)[i % 3], present=present))
    messages.append(big(10))
    tiles = sum(-(-(a * b) // tile) for a, b in [(ni, nj)] + [small] * (cap - 3) + [(ni, nj)])
    per = -(-tiles // cap)
    assert tiles == cap + 1 and per == 2 and cap % 2 == 0             # tiles (0, 1) in workgroup 0; (cap - 2, cap - 1) and (cap,) in the last two
    _, table = _check(messages, [bool(i % 2) for i in range(len(messages))], gpu_device)
    assert int(table["tile0"][1]) == 2 and int(table["tile0"][-1]) == cap - 1 and len(table) == cap - 1


def test_past_one_trip_of_a_wave_of_the_count_launch(gpu_device):
    """In the count launch a WAVE owns a tile and the four waves of a workgroup stride over its ceil(tiles / max_blocks) consecutive
    tiles by 4: a wave makes a second trip only with 5 tiles or more per workgroup, that is with more than 4 * max_blocks tiles.
    Thousands of one-tile fields -- two with a bitmap, one without, in turn -- and four bitmap fields of nine tiles: in its later
    trips a wave steps over several fields, or stays inside one; a workgroup of the unpack launch carries ranks through its tiles,
    changes field in every trip and meets a trip without barriers (no bitmap) between two trips with them."""
    tile, cap = _geometry()
    g = np.random.default_rng(77)
    small, (ni, nj) = (7, 3), (41, -(-(8 * tile + 100) // 41))
    assert -(-(ni * nj) // tile) == 9
    n_big, waves = 4, 4
    n_small = 5 * cap + 3 - 9 * n_big
    at_big = {10, 1000, 3001, 7000}
    messages, shapes, bitmapped = [], [], []
    for i in range(n_small + n_big):
        if i in at_big:
            a, b, with_bitmap, nbits = ni, nj, True, (9, 16, 12, 11)[len(shapes) % 4]
        else:
            a, b, with_bitmap, nbits = *small, i % 3 != 2, (16, 11, 5)[i % 3]
        present = (g.random(a * b) < 0.5) if with_bitmap else None
        messages.append(cases.random_message(g, a, b, nbits, 0.5 * (i % 9) - 2.0, -2, (0, 2, -1)[i % 3], present=present))
        shapes.append((a, b))
        bitmapped.append(with_bitmap)
    per_field = np.array([-(-(a * b) // tile) for a, b in shapes])
    tiles = int(per_field.sum())
    per = -(-tiles // cap)
    field_of_tile = np.repeat(np.arange(len(shapes)), per_field)
    assert tiles > waves * cap and per >= waves + 1                   # some wave of the count launch makes a second trip
    later = [t for t in range(tiles) if t % per >= waves]              # the tiles of those later trips; the wave's trip before: t - 4
    assert any(field_of_tile[t] - field_of_tile[t - waves] >= 2 and bitmapped[field_of_tile[t]] for t in later)      # steps over fields
    assert any(field_of_tile[t] == field_of_tile[t - waves] for t in later)                                            # stays in one
    runs = [[bitmapped[f] for f in field_of_tile[b * per:(b + 1) * per]] for b in range(-(-tiles // per))]
    assert any(any(r[j - 1] and not r[j] and r[j + 1] for j in range(1, len(r) - 1)) for r in runs)                  # bitmap, none, bitmap
    assert any(t % per and field_of_tile[t] == field_of_tile[t - 1] and bitmapped[field_of_tile[t]] for t in range(tiles))   # ranks carried on
    _, table = _check(messages, [bool(i % 2) for i in range(len(messages))], gpu_device)
    assert len(table) == len(messages) and int(table["tile0"][-1]) == tiles - 1


def test_count_below_the_bitmaps_population_is_clamped(gpu_device):
    """a descriptor that says fewer values than its bitmap has points goes straight through ops.grib_unpack: the points of rank >= count
    are NaN, the others exact.  The stream sits in the middle of a larger buffer."""
    from py4cast_amd import grib2

    tile, _ = _geometry()
    g = np.random.default_rng(4)
    ni, nj = 37, -(-(tile + 37) // 37)
    present = g.random(ni * nj) < 0.5
    surplus = 9
    messages = [cases.random_message(g, ni, nj, nbits, 1.5, -3, 1, present=present) for nbits in (16, 11)]
    fields = [grib2.field_of(m) for m in messages]

    def fewer(table):
        table["count"] -= surplus

    got, table, floats = _run(fields, [False, True], gpu_device, table_edit=fewer, lead=4096, tail=4096)
    assert (table["count"] == int(present.sum()) - surplus).all() and (table["stream_off"] >= 4096).all()
    planes = []
    for m, flip in zip(messages, (False, True)):
        plane = cases.expected_plane(m).reshape(-1).copy()
        plane[np.flatnonzero(present)[-surplus:]] = np.nan
        plane = plane.reshape(nj, ni)
        planes.append(plane[::-1] if flip else plane)
    assert cases.same_bits(got, cases.expected_buffer(table, planes, floats))


def test_refusals_write_nothing(gpu_device):
    """every error of the header's list returns non-zero before anything is launched"""
    from py4cast_amd import _lib as L
    from py4cast_amd import grib2, ops

    dev = gpu_device
    g = np.random.default_rng(6)
    ni, nj = 9, 5
    present = g.random(ni * nj) < 0.5
    fields = [grib2.field_of(cases.random_message(g, ni, nj, 12, 1.0, -1, 1)),
              grib2.field_of(cases.random_message(g, ni, nj, 12, 1.0, -1, 1, present=present))]
    buf, good, floats = cases.layout(fields)
    good["tile0"] = [0, 1]
    bytes_dev = torch.from_numpy(buf).to(dev)
    out = torch.full((floats,), float(cases.SENTINEL), dtype=torch.float32, device=dev)
    ws = torch.zeros(16, dtype=torch.int32, device=dev)
    handle = L.lib()

    def call(table, bytes_ptr=L.ptr(bytes_dev), nbytes=buf.size, out_ptr=L.ptr(out), ws_ptr=L.ptr(ws), host=True, device=True):
        table_dev = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
        rc = handle.p4c_grib_unpack(bytes_ptr, nbytes, L.ptr(table_dev) if device else None, ctypes.c_void_p(table.ctypes.data) if host else None,
                                    len(table), out_ptr, ws_ptr, L.stream(dev))
        torch.cuda.synchronize()
        return rc, (handle.p4c_last_error() or b"").decode()

    def edited(index, **columns):
        table = good.copy()
        for name, value in columns.items():
            table[index][name] = value
        return table

    N = ni * nj
    s1 = int(good[1]["stream_off"])
    bad = {      # what is wrong -> (the call, a fragment of the error only this refusal writes)
        "null bytes": (dict(table=good, bytes_ptr=None), "null pointer"), "null planes": (dict(table=good, out_ptr=None), "null pointer"),
        "null device table": (dict(table=good, device=False), "null pointer"), "null host table": (dict(table=good, host=False), "null pointer"),
        "null workspace with a bitmap": (dict(table=good, ws_ptr=None), "null workspace"),
        "nbits 33": (dict(table=edited(0, nbits=33)), "field 0: nbits = 33"), "nbits -1": (dict(table=edited(0, nbits=-1)), "field 0: nbits = -1"),
        "D 16": (dict(table=edited(0, D=16)), "field 0: nbits = 12, D = 16"), "D -16": (dict(table=edited(1, D=-16)), "field 1: nbits = 12, D = -16"),
        "count > points": (dict(table=edited(1, count=N + 1)), f"field 1: {N + 1} values for {N} points"),
        "no bitmap, count != points": (dict(table=edited(0, count=N - 1)), f"field 0: no bitmap and {N - 1} values"),
        "short stream": (dict(table=edited(0, stream_len=(N * 12 + 7) // 8 - 1)), f"field 0: a stream of {(N * 12 + 7) // 8 - 1} bytes"),
        "stream past the buffer": (dict(table=good, nbytes=s1 + int(good[1]["stream_len"]) - 1), f"field 1: the stream [{s1},"),
        "bitmap past the buffer": (dict(table=good, nbytes=int(good[1]["bitmap_off"]) + (N + 7) // 8 - 1), f"field 1: the bitmap [{int(good[1]['bitmap_off'])},"),
        "stream_off misaligned": (dict(table=edited(0, stream_off=2)), "field 0: stream_off = 2,"),
        "bitmap_off misaligned": (dict(table=edited(1, bitmap_off=int(good[1]["bitmap_off"]) + 2)), f"bitmap_off = {int(good[1]['bitmap_off']) + 2},"),
        "dst_off misaligned": (dict(table=edited(1, dst_off=int(good[1]["dst_off"]) + 2)), f"dst_off = {int(good[1]['dst_off']) + 2}:"),
        "bitmap_off -2": (dict(table=edited(0, bitmap_off=-2)), "bitmap_off = -2 (-1: no bitmap)"),
        "tile0": (dict(table=edited(1, tile0=2)), "field 1: tile0 = 2, the tiles before it are 1"),
        "2^31 points": (dict(table=edited(0, ni=65536, nj=32768)), f"field 0: {2 ** 31} points"),
        "bytes misaligned": (dict(table=good, bytes_ptr=ctypes.c_void_p(bytes_dev.data_ptr() + 1)), "must be 4-byte aligned"),
    }
    for what, (kw, fragment) in bad.items():
        rc, message = call(**kw)
        assert rc != 0 and "p4c_grib_unpack" in message and fragment in message, (what, message)
    assert bool((out == float(cases.SENTINEL)).all()), "a refused call wrote"
    rc, _ = call(good)                                                # the table the refusals were derived from is a good one
    assert rc == 0
    want = cases.expected_buffer(good, grib2.unpack_fields(fields), floats)
    assert cases.same_bits(out.cpu().numpy(), want)
    # the wrapper raises with the library's message
    with pytest.raises(L.P4CError, match="nbits = 33"):
        ops.grib_unpack(bytes_dev, edited(0, nbits=33), out=out)
    with pytest.raises(L.P4CError, match="holds every plane"):
        ops.grib_unpack(bytes_dev, good, out=out[:floats - cases.GUARD - 8])


def test_the_16_bit_path_equals_the_generic_one(gpu_device):
    """16 bits without a bitmap take the specialised path; the same stream under an all-ones bitmap takes the generic one"""
    from py4cast_amd import _lib as L

    handle = L.lib()
    assert handle.p4c_grib_unpack_fast(16, 0) == 1 and handle.p4c_grib_unpack_fast(16, 1) == 0
    tile, _ = _geometry()
    ni, nj = 37, -(-(tile + 37) // 37)
    X = np.random.default_rng(12).integers(0, 2 ** 16, size=ni * nj, dtype=np.uint64)
    X[:2] = (0, 2 ** 16 - 1)
    messages = [cases.message(ni, nj, X, 16, 271.25, -6, 2), cases.message(ni, nj, X, 16, 271.25, -6, 2, present=np.ones(ni * nj, dtype=bool))]
    for flip in (False, True):
        got, table = _check(messages, [flip, flip], gpu_device)
        a, b = (got[int(r["dst_off"]):int(r["dst_off"]) + ni * nj] for r in table)
        assert int(table[0]["bitmap_off"]) < 0 <= int(table[1]["bitmap_off"]) and np.array_equal(a.view(np.int32), b.view(np.int32))
