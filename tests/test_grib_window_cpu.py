"""
The windowed GRIB decode without a GPU: ``grib2.unpack_window`` (the contract of csrc/grib_window.hip in numpy) against
``grib2.decode`` followed by flip, crop and two float32 steps, bit for bit; ``grib2.window_slice``; the table ``datapipe.window_table``
builds from a plan, run through a numpy restatement of the kernel's indexing; the record's layout against the C header.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_unpack_cases as cases  # noqa: E402
import grib_window_cases as wc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NJ, NI = wc.NJ, wc.NI                                                  # 29 x 37
WINDOWS = [(3, 22, 5, 28), (0, 29, 0, 37), (17, 29, 30, 37)]           # the last one ends on the last row and the last column


@pytest.mark.parametrize("south_to_north", [False, True])
@pytest.mark.parametrize("nbits", wc.NBITS)
def test_unpack_window_equals_decode_flip_crop_standardise(nbits, south_to_north):
    from py4cast_amd import grib2

    g = np.random.default_rng(100 + nbits)
    for D in wc.DS:
        for E in (-3, 2):
            msg = cases.random_message(g, NI, NJ, nbits, float(np.float32(g.normal() * 30)), E, D, south_to_north=south_to_north)
            field = grib2.field_of(msg)
            for window in WINDOWS:
                for mean, std in ((0.0, 1.0), (3.25, 0.7)):
                    got = grib2.unpack_window(field, window, mean, std)
                    want = wc.expected_window(msg, window, mean, std)
                    assert got.dtype == np.float32 and cases.same_bits(got, want), (nbits, D, E, window, mean)
    if nbits:
        assert float(np.ptp(got)) > 0


@pytest.mark.parametrize("south_to_north", [False, True])
@pytest.mark.parametrize("nbits", [7, 12, 16, 31])
def test_window_slice(nbits, south_to_north):
    from py4cast_amd import grib2

    g = np.random.default_rng(7)
    msg = cases.random_message(g, NI, NJ, nbits, 2.5, -3, 1, south_to_north=south_to_north)
    field = grib2.field_of(msg)
    for r0, r1 in ((3, 22), (0, 29), (28, 29), (0, 1)):
        start, end, bit0 = grib2.window_slice(field, r0, r1)
        first, last = (NJ - r1, NJ - r0) if south_to_north else (r0, r1)          # stream rows
        lo_bit, hi_bit = first * NI * nbits, last * NI * nbits
        assert start % 4 == 0 and bit0 == 8 * start
        assert 8 * start <= lo_bit < 8 * start + 32                                # the rows' first bit lies in the slice's first word
        assert end == (hi_bit + 7) // 8 <= len(field.stream)                       # and its last byte holds their last bit
        for window in ((r0, r1, 0, NI), (r0, r1, 5, 28)):
            whole = grib2.unpack_window(field, window, 1.5, 2.0)
            sliced = grib2.unpack_window(field, window, 1.5, 2.0, data=bytes(field.stream[start:end]), bit0=bit0)
            assert cases.same_bits(sliced, whole) and cases.same_bits(whole, wc.expected_window(msg, window, 1.5, 2.0))
        if last < NJ:                                                              # the stream row after the slice is not in it
            after = (r0 - 1, r1, 0, NI) if south_to_north else (r0, r1 + 1, 0, NI)
            with pytest.raises(grib2.GribError, match="leave"):
                grib2.unpack_window(field, after, data=bytes(field.stream[start:end]), bit0=bit0)


def test_window_slice_of_a_row_that_starts_inside_a_byte():
    from py4cast_amd import grib2

    msg = cases.random_message(np.random.default_rng(3), NI, NJ, 7, -1.0, -2, 0)
    field = grib2.field_of(msg)
    assert (3 * NI * 7) % 8 == 1                                                   # row 3 starts at bit 1 of its byte
    start, end, bit0 = grib2.window_slice(field, 3, 5)
    assert (start, end, bit0) == (96, (5 * NI * 7 + 7) // 8, 768)
    got = grib2.unpack_window(field, (3, 5, 0, NI), data=bytes(field.stream[start:end]), bit0=bit0)
    assert cases.same_bits(got, wc.expected_window(msg, (3, 5, 0, NI)))
    zero = grib2.field_of(cases.random_message(np.random.default_rng(3), NI, NJ, 0, 4.0, 0, 0))
    assert grib2.window_slice(zero, 3, 5) == (0, 0, 0) and (grib2.unpack_window(zero, (3, 5, 1, 4)) == 4.0).all()


def test_fields_with_a_bitmap_and_bad_windows_are_refused():
    from py4cast_amd import grib2

    g = np.random.default_rng(4)
    present = g.random(NI * NJ) < 0.9
    masked = grib2.field_of(cases.random_message(g, NI, NJ, 12, 0.0, 0, 0, present=present))
    assert not grib2.window_qualifies(masked)
    with pytest.raises(grib2.GribError, match="bitmap"):
        grib2.window_slice(masked, 0, 4)
    with pytest.raises(grib2.GribError, match="bitmap"):
        grib2.unpack_window(masked, (0, 4, 0, 4))
    field = grib2.field_of(cases.random_message(g, NI, NJ, 12, 0.0, 0, 0))
    assert grib2.window_qualifies(field)
    with pytest.raises(grib2.GribError):
        grib2.window_slice(field, 5, 30)
    with pytest.raises(grib2.GribError):
        grib2.unpack_window(field, (0, 4, 30, 38))


def _run_table(rec, buf, H, W):
    """the indexing of grib_window_pack_kernel on one record, in numpy: stream point, bit in the slice, the value"""
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    p = (int(rec["row0"]) + y * int(rec["row_step"])) * int(rec["ni"]) + int(rec["col0"]) + x
    nbits = int(rec["nbits"])
    bits = np.unpackbits(buf[int(rec["slice_off"]):int(rec["slice_off"]) + int(rec["slice_len"])])
    at = (p * nbits - int(rec["bit0"])).reshape(-1)
    assert at.min() >= 0 and at.max() + nbits <= bits.size
    X = (bits[at[:, None] + np.arange(nbits)].astype(np.uint64) << np.arange(nbits - 1, -1, -1, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    v = ((float(rec["R"]) + np.ldexp(X.astype(np.float64), int(rec["E"]))) / 10.0 ** int(rec["D"])).astype(np.float32)
    return ((v - rec["mean"]) / rec["std"]).reshape(H, W)


@pytest.mark.parametrize("flip_lat", [True, False])
def test_the_table_of_a_plan_points_at_the_plans_pixels(flip_lat):
    """what ``load_native_batch`` selects through an identity plan -- rows flipped with ``flip_lat``, the sub-domain's origin -- in both
    scanning directions, from slices laid out in one buffer"""
    from py4cast_amd import datapipe, grib2, regrid

    g = np.random.default_rng(12)
    sub = (4, 23, 6, 29)
    plan = regrid.RegridPlan((NJ, NI), (NJ, NI), subdomain=sub, flip_lat=flip_lat)
    rows = datapipe.window_rows(plan)
    assert rows == ((NJ - sub[1], NJ - sub[0]) if flip_lat else (sub[0], sub[1]))
    specs = [(12, 1.0, -2, 1), (7, -3.0, 0, 0)]
    msgs = wc.messages(g, 2, 2, specs)
    fields = [[[grib2.field_of(m) for m in per_b] for per_b in per_f] for per_f in msgs]
    buf, places = wc.slices_buffer(fields, rows, 0xEE)
    table = datapipe.window_table(fields, places, ["a", "b"], plan)
    assert table.fields.shape == (2, 2, 2) and table.shape == (19, 23) and table.names == ("a", "b")
    assert (table.fields["slice_off"] % 4 == 0).all() and (table.fields["bitmap_off"] == -1).all()
    for f in range(2):
        for b in range(2):
            for t in range(2):
                full = wc.expected_window(msgs[f][b][t], (0, NJ, 0, NI))
                want = (full[::-1] if flip_lat else full)[sub[0]:sub[1], sub[2]:sub[3]]
                assert cases.same_bits(_run_table(table.fields[b, t, f], buf, 19, 23), want), (f, b, t)
    # a resizing plan, a field of another size and a field with a bitmap have no window table
    with pytest.raises(ValueError, match="resizes"):
        datapipe.window_rows(regrid.RegridPlan((NJ, NI), (40, 50)))
    other = grib2.field_of(cases.random_message(g, 20, 20, 8, 0.0, 0, 0))
    assert not datapipe.window_qualifies(other, plan) and datapipe.window_qualifies(fields[0][0][0], plan)
    with pytest.raises(ValueError, match="not a simple-packed field"):
        datapipe.window_table([[[other]]], [[[(0, 4, 0)]]], ["a"], plan)


def test_the_record_mirrors_the_header():
    from py4cast_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "py4cast_hip.h")).read()
    body = re.search(r"typedef struct p4c_grib_wfield \{(.*?)\} p4c_grib_wfield;", header, re.S).group(1)
    names = []
    for line in body.splitlines():
        decl = line.split("/*")[0].strip().rstrip(";")
        if decl:
            names += [n.strip() for n in decl.split(None, 1)[1].split(",")]
    assert tuple(names) == ops.GRIB_WFIELD.names and ops.GRIB_WFIELD.itemsize == 72
    proto = re.search(r"int p4c_grib_window_pack\((.*?)\);", header, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["p4c_grib_window_pack"]) == 11
    assert "p4c_grib_window_max_features" in _lib.OTHER and ops.GRIB_WINDOW_MAX_FEATURES == 144
    rec = ops.grib_wfields([{"slice_off": 8, "nbits": 16}])
    assert rec["bitmap_off"][0] == -1 and rec["row_step"][0] == 1 and rec["std"][0] == 1.0 and rec["slice_off"][0] == 8
    with pytest.raises(_lib.P4CError, match="no column"):
        ops.grib_wfields([{"stream_off": 0}])
