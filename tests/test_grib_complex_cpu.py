"""
Complex packing (GRIB2 templates 5.2 / 5.3) on the host: ``grib2.complex_field_of``, ``decode``, ``unpack_fields`` and the host path
of ``diskio.GribPlaneReader``, against the integers handed to the encoder of tests/grib_complex_cases.py, bit for bit, and against
the worked example of the format as literal bytes.  No GPU.
"""
import dataclasses
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib2_reference as ref  # noqa: E402
import grib_complex_cases as cc  # noqa: E402
import grib_unpack_cases as cases  # noqa: E402

# the worked example: template 5.3, order 2, nbytes 1, 10 values, R = 250, E = -1, D = 1, 3 groups of widths (0, 0, 3) and lengths
# (2, 3, 5); the last scaled length is stored as 1 and must be ignored
EXAMPLE_S5 = bytes.fromhex("00 00 00 31 05 00 00 00 0a 00 03 43 7a 00 00 80 01 00 01 03 00 01 00 00 00 00 00 00 00 00 00"
                           "00 00 00 03 00 02 00 00 00 02 01 00 00 00 05 01 02 01")
EXAMPLE_PAYLOAD = bytes.fromhex("64 67 86 1c 00 0c 60 1a da")
EXAMPLE_F = [100, 103, 107, 112, 118, 118, 118, 117, 115, 112]
EXAMPLE_BITS = [0x41f00000, 0x41f13333, 0x41f2cccd, 0x41f4cccd, 0x41f73333, 0x41f73333, 0x41f73333, 0x41f6cccd, 0x41f60000, 0x41f4cccd]


def example_message():
    return cc.assemble(5, 2, EXAMPLE_S5, EXAMPLE_PAYLOAD)


def _bits(plane):
    return [int(v) for v in np.asarray(plane, dtype=np.float32).reshape(-1).view(np.uint32)]


def test_the_worked_example():
    from py4cast_amd import grib2

    msg = example_message()
    f = grib2.complex_field_of(msg)
    assert (f.ni, f.nj, f.count, f.R, f.E, f.D, f.scanning_mode) == (5, 2, 10, 250.0, -1, 1, 0)
    assert (f.ng, f.ref_bits, f.w_ref, f.w_bits, f.l_ref, f.l_inc, f.l_last, f.l_bits, f.order, f.nbytes) == (3, 3, 0, 2, 2, 1, 5, 1, 2, 1)
    assert (f.ival1, f.ival2, f.gmin, f.template) == (100, 103, -6, 3) and f.bitmap is None
    assert f.stream.obj is grib2.Message(msg).sections[7] or bytes(f.stream) == EXAMPLE_PAYLOAD
    assert [int(v) for v in grib2.complex_integers(f)] == EXAMPLE_F
    assert _bits(grib2.decode(msg)[0].filled(np.nan).astype(np.float32)) == EXAMPLE_BITS
    assert _bits(grib2.unpack_fields([f])[0]) == EXAMPLE_BITS
    integers, plane = cc.restate(msg)
    assert integers == EXAMPLE_F and _bits(plane) == EXAMPLE_BITS
    assert _bits(cc.expected_plane(EXAMPLE_F, 5, 2, 250.0, -1, 1)) == EXAMPLE_BITS
    # and the encoder of the tests writes these very bytes
    numbers, payload, X = cc.encode(EXAMPLE_F, 2, [0, 2, 5], nbytes=1, ref_bits=3, w_ref=0, w_bits=2, l_ref=2, l_inc=1, l_bits=1, last_stored=1)
    assert payload == EXAMPLE_PAYLOAD and X == [0, 0, 7, 7, 7, 0, 6, 5, 5, 5] and cc.section5(10, 250.0, -1, 1, numbers) == EXAMPLE_S5


def host_cases():
    """name -> (ni, nj, f, order, bounds, R, E, D, present, south_to_north, encode parameters)"""
    g = np.random.default_rng(52)
    out = {}
    for order in (0, 1, 2):
        n = 23 * 13
        f = cc.smooth_field(g, n, offset=3000 if order == 0 else -40)
        out[f"order{order}"] = (23, 13, f, order, cc.random_bounds(g, n), 250.0, -1, 1, None, False, {})
        present = g.random(23 * 13) < 0.6
        fm = f[:int(present.sum())]
        out[f"order{order}_bitmap_s2n"] = (23, 13, fm, order, cc.random_bounds(g, fm.size), -3.5, -2, -1, present, True, {})
    f, bounds = cc.wide_field()
    out["widths_0_1_31_32"] = (6, 3, f, 0, bounds, 0.0, 0, 0, None, False, dict(ref_bits=32, w_bits=6))
    f = g.integers(0, 500, size=40)
    out["ref_bits_0"] = (8, 5, f, 0, [0, 7, 20], 1.0, 0, 0, None, False, dict(ref_bits=0, w_bits=4))
    out["w_bits_0"] = (8, 5, f, 0, [0, 7, 20], 1.0, 0, 2, None, False, dict(w_ref=9, w_bits=0))
    out["l_bits_0"] = (8, 5, cc.smooth_field(g, 40), 1, list(range(0, 40, 7)), 1.0, 1, 0, None, False, dict(l_ref=7, l_bits=0))
    out["l_inc_3"] = (8, 5, cc.smooth_field(g, 40), 2, [0, 2, 7, 21, 29], 1.0, 0, 0, None, False, dict(l_ref=2, l_inc=3, l_bits=3))
    out["last_length_disagrees"] = (8, 5, cc.smooth_field(g, 40), 1, [0, 10, 20], 1.0, 0, 0, None, False, dict(last_stored=3))
    out["negative_descriptors"] = (8, 5, cc.smooth_field(g, 40, offset=-9000), 2, [0, 13], 1.0, 0, 0, None, False, {})
    zero = np.concatenate([[0, 0], np.cumsum(np.cumsum(g.integers(0, 9, size=38)))])
    out["nbytes0"] = (8, 5, zero, 2, [0, 16], 2.0, 0, 0, None, False, dict(nbytes=0, gmin=0))
    out["nbytes0_order1"] = (8, 5, np.concatenate([[0], np.cumsum(g.integers(0, 9, size=39))]), 1, [0, 16], 2.0, 0, 0, None, False,
                             dict(nbytes=0, gmin=0))
    small = (40 + 30 * np.sin(np.arange(40) / 9.0)).astype(np.int64)
    out["nbytes1"] = (8, 5, small, 2, [0, 16], 2.0, 0, 0, None, False, dict(nbytes=1))
    out["nbytes3"] = (8, 5, cc.smooth_field(g, 40, offset=-4_000_000), 2, [0, 16], 2.0, 0, 0, None, False, dict(nbytes=3))
    out["nbytes4"] = (8, 5, cc.smooth_field(g, 40, offset=1_500_000_000), 1, [0, 16], 2.0, -3, 0, None, False, dict(nbytes=4))
    out["count1_order2"] = (1, 1, np.array([-77]), 2, [0], 2.0, 0, 0, None, False, {})
    out["count2_order2"] = (2, 1, np.array([-77, 12]), 2, [0], 2.0, 0, 0, None, False, {})
    out["one_group"] = (8, 5, cc.smooth_field(g, 40), 2, [0], 2.0, 0, 0, None, False, {})
    out["empty_groups"] = (8, 5, cc.smooth_field(g, 40), 1, [0, 0, 5, 5, 5, 9, 40], 2.0, 0, 0, None, False, {})
    out["placeholders_ignored"] = (8, 5, cc.smooth_field(g, 40), 2, [0, 9], 2.0, 0, 0, None, False, dict(placeholder=5))
    out["wrap"] = (35, 20, cc.wrap_field(g, 700), 2, cc.random_bounds(g, 700), 0.0, -20, 0, None, False, dict(nbytes=4, ref_bits=32))
    present = cases.window_present(9, 7, 1, 5, 2, 6)
    out["window_bitmap"] = (9, 7, cc.smooth_field(g, 25), 2, [0, 4, 11], 2.0, 0, 1, present, False, {})
    return out


HOST_CASES = host_cases()


@pytest.mark.parametrize("name", list(HOST_CASES))
def test_decode_and_unpack_fields_give_the_encoders_integers(name):
    from py4cast_amd import grib2

    ni, nj, f, order, bounds, R, E, D, present, s2n, params = HOST_CASES[name]
    msg = cc.message(ni, nj, f, order, bounds, R, E, D, present=present, south_to_north=s2n, **params)
    want = cc.expected_plane(f, ni, nj, R, E, D, present=present)
    with np.errstate(all="ignore"):
        decoded = grib2.decode(msg)[0]
    assert cases.same_bits(decoded.filled(np.nan).astype(np.float32), want)
    assert np.array_equal(decoded.mask.reshape(-1), np.zeros(ni * nj, dtype=bool) if present is None else ~np.asarray(present))
    field = grib2.complex_field_of(msg)
    assert field.order == order and field.template == (3 if order else 2) and field.south_to_north == s2n
    assert [int(v) for v in grib2.complex_integers(field)] == [int(v) for v in f]
    assert cases.same_bits(grib2.unpack_fields([field])[0], want)
    assert cases.same_bits(grib2.unpack_fields([field], flip=True)[0], cc.expected_plane(f, ni, nj, R, E, D, present=present, flip=True))
    integers, plane = cc.restate(msg)
    assert integers == [int(v) for v in f] and cases.same_bits(plane, want)


def test_the_wrap_field_passes_2_to_the_32():
    f = HOST_CASES["wrap"][2]
    d = f[2:] - 2 * f[1:-1] + f[:-2]
    assert np.abs(np.cumsum(d)).max() > 2 ** 32 and np.abs(np.cumsum(d * np.arange(2, f.size))).max() > 2 ** 40


def test_a_count_below_the_bitmaps_population():
    from py4cast_amd import grib2

    g = np.random.default_rng(8)
    ni, nj = 9, 7
    present = g.random(ni * nj) < 0.5
    n = int(present.sum())
    f = cc.smooth_field(g, n)
    field = grib2.complex_field_of(cc.message(ni, nj, f, 2, [0, 6, 15], 2.0, -1, 1, present=present))
    more = present.copy()
    more[np.flatnonzero(~present)[:5]] = True                 # five more points present than values packed
    wider = dataclasses.replace(field, bitmap=memoryview(np.packbits(more).tobytes()))
    for flip in (False, True):
        want = cc.expected_plane(f, ni, nj, 2.0, -1, 1, present=more, flip=flip, count=n)
        assert int(np.isnan(want).sum()) == ni * nj - n and cases.same_bits(grib2.unpack_fields([wider], flip=flip)[0], want)


def _s5(change):
    return lambda s: change(s)


def test_complex_field_of_refusals_name_the_octet():
    from py4cast_amd import grib2

    g = np.random.default_rng(3)
    ni, nj = 9, 5
    present = g.random(ni * nj) < 0.5
    f = cc.smooth_field(g, ni * nj)
    plain = cc.message(ni, nj, f, 2, [0, 11, 30], 1.5, -2, 1)
    plain52 = cc.message(ni, nj, f + 3000, 0, [0, 11, 30], 1.5, -2, 1)
    masked = cc.message(ni, nj, f[:int(present.sum())], 1, [0, 11], 1.5, -2, 1, present=present)
    assert grib2.complex_field_of(plain).count == ni * nj and grib2.complex_field_of(masked).count == int(present.sum())
    set_octet = lambda octet, value: (lambda s: s.__setitem__(octet - 1, value))   # noqa: E731

    def refused(pattern, msg):
        with pytest.raises(grib2.GribError, match=pattern):
            grib2.complex_field_of(msg)

    for number in (0, 40, 41, 42):
        refused(rf"section 5 octets 10-11.*5\.{number};", cc.patched(plain, 5, lambda s, n=number: s.__setitem__(slice(9, 11), struct.pack(">H", n))))
    refused("section 5 octets 10-11", cases.random_message(g, ni, nj, 12, 1.5, -2, 1))
    refused("section 5 octets 1-4: 48 octets", cc.patched(plain, 5, lambda s: s[:-1]))
    refused("section 5 octets 1-4: 46 octets", cc.patched(plain52, 5, lambda s: s[:-1]))
    for octet in (20, 37, 47):
        refused(rf"section 5 octet {octet}: 33 bits", cc.patched(plain, 5, set_octet(octet, 33)))
        grib2.complex_field_of(cc.patched(plain52, 5, set_octet(octet, 32)))       # 32 bits pass the header (the tables still fit)
    refused("section 5 octet 22: group splitting method 0", cc.patched(plain, 5, set_octet(22, 0)))
    refused("section 5 octet 22: group splitting method 2", cc.patched(plain52, 5, set_octet(22, 2)))
    for management in (1, 2):
        refused(rf"section 5 octet 23: missing value management {management}", cc.patched(plain, 5, set_octet(23, management)))
    for order in (0, 3):
        refused(rf"section 5 octet 48: spatial differencing of order {order}", cc.patched(plain, 5, set_octet(48, order)))
    refused("section 5 octet 49: 5 octets", cc.patched(plain, 5, set_octet(49, 5)))
    refused("section 5 octets 32-35: no group", cc.patched(plain, 5, lambda s: s.__setitem__(slice(31, 35), bytes(4))))
    refused("section 5 octets 18-19: D = 16", cc.patched(plain, 5, lambda s: s.__setitem__(slice(17, 19), ref.sm(16, 2))))
    refused("section 5 octets 18-19: D = -16", cc.patched(plain52, 5, lambda s: s.__setitem__(slice(17, 19), ref.sm(-16, 2))))
    refused("section 6 octet 6: bitmap indicator 254", cc.patched(plain, 6, lambda s: s.__setitem__(5, 254)))
    n = int(present.sum())
    refused(rf"section 5 octets 6-9: {n - 1} values for {n} points present",
            cc.patched(masked, 5, lambda s: s.__setitem__(slice(5, 9), struct.pack(">I", n - 1))))
    refused(rf"section 5 octets 6-9: {ni * nj - 1} values for {ni * nj} points and no bitmap",
            cc.patched(plain, 5, lambda s: s.__setitem__(slice(5, 9), struct.pack(">I", ni * nj - 1))))
    refused("section 6 octets 1-4", cc.patched(masked, 6, lambda s: s[:-1]))
    # section 7 must hold the descriptors and the three padded tables: 3 + ceil(3*16/8) + ceil(3*6/8) + ceil(3*8/8) = 15 octets
    tables = grib2.complex_field_of(plain).table_bits()[3] // 8
    assert tables == 3 * 2 + 6 + 3 + 3
    refused("section 7 octets 1-4", cc.patched(plain, 7, lambda s: s[:5 + tables - 1]))
    grib2.complex_field_of(cc.patched(plain, 7, lambda s: s[:5 + tables]))          # the values are the device's (and unpack_fields') to check
    first = lambda data: grib2.Message(data[:struct.unpack_from(">Q", data, 8)[0]])   # noqa: E731
    for bit in (0x80, 0x20, 0x10):     # what check_grid refuses
        with pytest.raises(grib2.GribError, match=rf"section 3 octet 72.*0x{bit:02x}"):
            grib2.complex_field_of(first(ref.template_file(scan_extra=bit, data_template=3)))
    with pytest.raises(grib2.GribError, match="section 3 octets 13-14.*3.30"):
        grib2.complex_field_of(first(ref.template_file(grid_template=30)))
    # nbytes 0: the three descriptors are 0
    zero = cc.message(ni, nj, np.zeros(ni * nj, dtype=np.int64), 2, [0], 1.5, 0, 0, nbytes=0, gmin=0)
    field = grib2.complex_field_of(zero)
    assert (field.nbytes, field.ival1, field.ival2, field.gmin) == (0, 0, 0, 0)
    # field_of keeps refusing them, decode reads them
    with pytest.raises(grib2.GribError, match=r"section 5 octets 10-11.*5\.3;.*out of scope"):
        grib2.field_of(plain)
    assert grib2.decode(plain)[0].shape == (nj, ni)


@pytest.mark.parametrize("kind", ["lengths", "width", "stream"])
def test_unpack_fields_raises_for_a_stream_that_contradicts_its_header(kind, tmp_path):
    from py4cast_amd import grib2
    from py4cast_amd.diskio import GribPlaneReader

    msg, _, words = cc.malformed(kind)
    field = grib2.complex_field_of(msg)                       # the header alone is in order
    with pytest.raises(grib2.GribError, match=words):
        grib2.unpack_fields([field])
    with pytest.raises(grib2.GribError, match=words):
        grib2.decode(msg)
    with pytest.raises(AssertionError):
        cc.restate(msg)
    path = tmp_path / "bad.grib"
    path.write_bytes(msg)
    with pytest.raises(grib2.GribError, match=re.escape(str(path)) + ".*" + words):
        GribPlaneReader(device=None).read([[[(path, {"discipline": 0, "parameterCategory": 0, "parameterNumber": 0})]]])


def test_gribfile_hands_out_either_kind_from_one_file(tmp_path):
    from py4cast_amd import grib2

    data, fids, _ = cc.mixed_file(False)
    path = tmp_path / "mixed.grib"
    path.write_bytes(data)
    gfile = grib2.GribFile(path)
    kinds = [type(gfile.field(fid)[1]) for fid in fids]
    assert kinds == [grib2.PackedField, grib2.ComplexField, grib2.ComplexField, grib2.ComplexField]
    assert [gfile.field(fid)[1].order for fid in fids[1:]] == [0, 1, 2] and gfile.field(fids[2])[1] is gfile.field(fids[2])[1]
    bad = tmp_path / "bad.grib"
    bad.write_bytes(cc.patched(data[len(data) - len(grib2.parse_messages(data)[-1].raw):], 5, lambda s: s.__setitem__(22, 1)))
    with pytest.raises(grib2.GribError, match=re.escape(str(bad)) + ": section 5 octet 23"):
        grib2.GribFile(bad).field(fids[-1])


@pytest.mark.parametrize("south_to_north", [False, True])
def test_the_host_reader_on_a_file_that_mixes_the_templates(south_to_north, tmp_path):
    from py4cast_amd.diskio import GribPlaneReader

    data, fids, planes = cc.mixed_file(south_to_north)
    path = tmp_path / "mixed.grib"
    path.write_bytes(data)
    got, lat, lon = GribPlaneReader(device=None).read([[[(path, fid)]] for fid in fids])
    assert tuple(got.shape) == (4, 1, 1, 23, 39) and lat[0] > lat[-1]
    for i, want in enumerate(planes):
        assert cases.same_bits(got[i, 0, 0].numpy(), want), i
    assert np.isnan(got[2].numpy()).any() and not np.isnan(got[3].numpy()).any()


def test_the_record_mirrors_the_header():
    """GRIB_CFIELD against p4c_grib_cfield as the header declares it: the same names in the same order, natural alignment without
    holes, and the launch constants the library reports"""
    from py4cast_amd import ops

    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "py4cast_hip.h")).read()
    body = re.search(r"typedef struct p4c_grib_cfield \{(.*?)\} p4c_grib_cfield;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"int64_t": ("<i8", 8), "int32_t": ("<i4", 4), "uint32_t": ("<u4", 4), "float": ("<f4", 4)}
    declared, offset = [], 0
    for ctype, names in re.findall(r"(\w+)\s+([\w\s,]+);", body):
        for name in (n.strip() for n in names.split(",")):
            code, size = sizes[ctype]
            assert offset % size == 0, f"{name} is not naturally aligned"
            declared.append((name, code, offset))
            offset += size
    assert offset % 8 == 0 and ops.GRIB_CFIELD.itemsize == offset == 136
    assert [(n, ops.GRIB_CFIELD.fields[n][0].str, ops.GRIB_CFIELD.fields[n][1]) for n in ops.GRIB_CFIELD.names] == declared
    assert (ops.GRIB_STATUS_LENGTHS, ops.GRIB_STATUS_WIDTH, ops.GRIB_STATUS_STREAM) == (1, 2, 4)
    from py4cast_amd import _lib

    lib = _lib.lib()
    assert (lib.p4c_grib_complex_tile(), lib.p4c_grib_complex_chunk(), lib.p4c_grib_complex_max_blocks()) == \
        (ops.GRIB_COMPLEX_TILE, ops.GRIB_COMPLEX_CHUNK, ops.GRIB_COMPLEX_MAX_BLOCKS)
    assert lib.p4c_grib_unpack_complex_workspace_bytes(0, 0, 0) == 0
    small, big = lib.p4c_grib_unpack_complex_workspace_bytes(3, 2, 0), lib.p4c_grib_unpack_complex_workspace_bytes(3, 2, 1)
    assert small == 2 * 24 + 2 * ops.GRIB_COMPLEX_CHUNK * 12 + 3 * 16 + 3 * 4 and big == small + 3 * ops.GRIB_COMPLEX_TILE * 4
