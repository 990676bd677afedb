"""
Reading GRIB2 without a GPU: ``grib2.field_of`` / ``GribFile`` / ``unpack_fields`` (the contract of csrc/grib_unpack.hip in numpy) and
``diskio.GribPlaneReader(device=None)``.  The expected planes are ``grib2.decode`` of the same message rounded to float32, compared
bit for bit (tests/grib_unpack_cases.py); ``decode`` itself is checked against exact rationals in tests/test_grib2_cpu.py.
"""
import dataclasses
import datetime as dt
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib2_reference as ref  # noqa: E402
import grib_unpack_cases as cases  # noqa: E402

FIELD_OF = {"aro_t2m_2m": 0, "aro_u10_10m": 1, "aro_prmsl_0hpa": 4, "aro_tp_0m": 5, "aro_r2_2m": 3}    # index into ref.FIELDS


def _fid(name):
    from py4cast_amd.outputs import grib_fid

    return grib_fid(name, 3600)[0]


def _patched(msg, number, change):
    """the message with ``change(bytearray of section `number`)`` applied (it may return a new bytearray); lengths are fixed up"""
    sections = ref.walk(msg)[0]
    parts = []
    for n in sorted(k for k in sections if k != 0):
        s = bytearray(sections[n])
        if n == number:
            s = change(s) or s
            s[0:4] = struct.pack(">I", len(s))
        parts.append(bytes(s))
    return bytes(sections[0][:8]) + struct.pack(">Q", 20 + sum(len(p) for p in parts)) + b"".join(parts) + b"7777"


def test_field_of_every_template_message_in_both_scan_directions():
    from py4cast_amd import grib2

    for south_to_north in (True, False):
        data = ref.template_file(south_to_north)
        messages, walked = grib2.parse_messages(data), ref.walk(data)
        assert len(messages) == len(ref.FIELDS)
        for m, sections in zip(messages, walked):
            f, k = grib2.field_of(m), ref.keys(sections)
            assert (f.ni, f.nj, f.count, f.nbits, f.E, f.D, f.scanning_mode) == (k["ni"], k["nj"], k["count"], k["nbits"], k["E"], k["D"], k["scan"])
            assert np.float32(f.R) == np.float32(k["R"]) and f.south_to_north == south_to_north and f.bitmap is None
            assert isinstance(f.stream, memoryview) and f.stream.obj is m.sections[7] and bytes(f.stream) == sections[7][5:]    # no copy
            assert cases.same_bits(grib2.unpack_fields([f])[0], cases.expected_plane(m))
            assert cases.same_bits(grib2.unpack_fields([f], flip=True)[0], cases.expected_plane(m, flip=True))
    # with a bitmap: what the writer emits for a sub-window
    m = messages[0]
    h, w = 5, 7
    _, _, R, E, _, stream = ref.pack(np.arange(h * w, dtype=np.float32), 2, 16)
    windowed = grib2.Message(grib2.encode(m, ref.BASIS, dt.timedelta(hours=1), window=(3, 3 + h - 1, 2, 2 + w - 1), packed=stream, R=float(R),
                                          E=E, D=2, nbits=16))
    f = grib2.field_of(windowed)
    assert f.count == h * w and f.bitmap.obj is windowed.sections[6] and len(f.bitmap) == (ref.NI * ref.NJ + 7) // 8
    got = grib2.unpack_fields([f])[0]
    assert cases.same_bits(got, cases.expected_plane(windowed)) and int(np.isnan(got).sum()) == ref.NI * ref.NJ - h * w
    assert np.allclose(got[3:3 + h, 2:2 + w].reshape(-1), np.arange(h * w), atol=0.01)


def test_field_of_refusals_name_the_octet():
    from py4cast_amd import grib2

    g = np.random.default_rng(3)
    ni, nj = 9, 5
    present = g.random(ni * nj) < 0.5
    plain = cases.random_message(g, ni, nj, 12, 1.5, -2, 1)
    masked = cases.random_message(g, ni, nj, 12, 1.5, -2, 1, present=present)
    assert grib2.field_of(plain).count == ni * nj and grib2.field_of(masked).count == int(present.sum())
    for number in (2, 3, 40, 41, 42):
        with pytest.raises(grib2.GribError, match=rf"section 5 octets 10-11.*5\.{number};.*out of scope"):
            grib2.field_of(_patched(plain, 5, lambda s, n=number: s.__setitem__(slice(9, 11), struct.pack(">H", n))))
    with pytest.raises(grib2.GribError, match="section 5 octets 10-11"):
        grib2.field_of(grib2.parse_messages(ref.template_file(data_template=3))[0])
    with pytest.raises(grib2.GribError, match="section 6 octet 6: bitmap indicator 254"):
        grib2.field_of(_patched(plain, 6, lambda s: s.__setitem__(5, 254)))
    with pytest.raises(grib2.GribError, match="section 5 octet 20: 33 bits"):
        grib2.field_of(_patched(plain, 5, lambda s: s.__setitem__(19, 33)))
    with pytest.raises(grib2.GribError, match="section 5 octets 18-19: D = 16"):
        grib2.field_of(_patched(plain, 5, lambda s: s.__setitem__(slice(17, 19), ref.sm(16, 2))))
    with pytest.raises(grib2.GribError, match=rf"section 5 octets 6-9: {present.sum() - 1} values for {present.sum()} points present"):
        grib2.field_of(cases.message(ni, nj, np.zeros(int(present.sum())), 12, 0.0, 0, 0, present=present, count=int(present.sum()) - 1))
    with pytest.raises(grib2.GribError, match=rf"section 5 octets 6-9: {ni * nj - 1} values for {ni * nj} points and no bitmap"):
        grib2.field_of(cases.message(ni, nj, np.zeros(ni * nj), 12, 0.0, 0, 0, count=ni * nj - 1))
    with pytest.raises(grib2.GribError, match="section 7 octets 1-4"):
        grib2.field_of(_patched(plain, 7, lambda s: s[:-1]))
    with pytest.raises(grib2.GribError, match="section 6 octets 1-4"):
        grib2.field_of(_patched(masked, 6, lambda s: s[:-1]))
    # the padding bits of the bitmap's last octet do not count
    padded = _patched(masked, 6, lambda s: s.__setitem__(len(s) - 1, s[-1] | 0x07))           # 45 points: 3 padding bits
    assert grib2.field_of(padded).count == int(present.sum())
    first = lambda data: grib2.Message(data[:struct.unpack_from(">Q", data, 8)[0]])   # noqa: E731
    for bit in (0x80, 0x20, 0x10):     # what check_grid refuses
        with pytest.raises(grib2.GribError, match=rf"section 3 octet 72.*0x{bit:02x}"):
            grib2.field_of(first(ref.template_file(scan_extra=bit)))
    with pytest.raises(grib2.GribError, match="section 3 octets 13-14.*3.30"):
        grib2.field_of(first(ref.template_file(grid_template=30)))
    # decode refuses the same messages
    for bad in (_patched(plain, 6, lambda s: s.__setitem__(5, 254)), _patched(plain, 5, lambda s: s.__setitem__(slice(9, 11), struct.pack(">H", 2)))):
        with pytest.raises(grib2.GribError):
            grib2.decode(bad)


def test_gribfile_finds_what_template_finds(tmp_path):
    from py4cast_amd import grib2

    for south_to_north in (True, False):
        path = tmp_path / f"file_{south_to_north}.grib"
        path.write_bytes(ref.template_file(south_to_north))
        template, gfile = grib2.Template(path), grib2.GribFile(path)
        assert len(gfile.messages) == len(template.messages) == len(ref.FIELDS)
        for name, index in FIELD_OF.items():
            fid = _fid(name)
            assert gfile.messages.index(gfile.find(fid)) == template.messages.index(template.find(fid)) == index, name
            m, f = gfile.field(fid)
            assert m is gfile.messages[index] and gfile.field(fid)[1] is f                    # parsed once
        for finder in (template, gfile):
            with pytest.raises(grib2.GribError, match="not matched"):
                finder.find({"paramId": 167})
            with pytest.raises(KeyError, match="no message"):
                finder.find({"discipline": 0, "parameterCategory": 19, "parameterNumber": 1})
            assert finder.find({"shortName": "ignored", "parameterCategory": 3, "parameterNumber": 1}) is finder.messages[4]
        with pytest.raises(grib2.GribError, match="matching by shortName .* is out of scope"):      # the reference's way of selecting
            gfile.find({"shortName": "2t"})
    empty = tmp_path / "empty.grib"
    empty.write_bytes(b"")
    with pytest.raises(grib2.GribError, match="no GRIB2 message"):
        grib2.GribFile(empty)


@pytest.mark.parametrize("bitmap", [False, True])
def test_unpack_fields_equals_decode_at_every_width(bitmap):
    from py4cast_amd import grib2

    g = np.random.default_rng(17 + bitmap)
    ni, nj = 37, 5
    for nbits in range(33):
        present = (g.random(ni * nj) < 0.5) if bitmap else None
        R = np.float32((-1) ** nbits * (0.37 + nbits))
        msg = cases.random_message(g, ni, nj, nbits, float(R), int(g.integers(-30, 12)), (0, 2, -1)[nbits % 3], present=present)
        f = grib2.field_of(msg)
        assert f.nbits == nbits and (f.bitmap is not None) == bitmap
        want = cases.expected_plane(msg)
        assert cases.same_bits(grib2.unpack_fields([f])[0], want), nbits
        assert cases.same_bits(grib2.unpack_fields([f], flip=[True])[0], want[::-1]), nbits
        if nbits == 0:        # a constant field: R / 10^D wherever a point is present
            D = f.D
            const = np.float32(np.float64(R) / 10.0 ** D if D >= 0 else np.float64(R) * 10.0 ** -D)
            assert len(f.stream) == 0 and np.all(want[~np.isnan(want)] == const)
    # a descriptor that says fewer values than the bitmap has points: the surplus ranks are NaN, the rest unchanged
    present = g.random(ni * nj) < 0.5
    msg = cases.random_message(g, ni, nj, 11, 2.5, -3, 1, present=present)
    f, want = grib2.field_of(msg), cases.expected_plane(msg).reshape(-1).copy()
    short = dataclasses.replace(f, count=f.count - 7)
    want[np.flatnonzero(present)[-7:]] = np.nan
    assert cases.same_bits(grib2.unpack_fields([short])[0].reshape(-1), want)
    with pytest.raises(ValueError, match="flip flags"):
        grib2.unpack_fields([f], flip=[True, False])


def _files(tmp_path):
    """two dates x two scan directions of the builder's template file -> {(date index, south_to_north): path}"""
    out = {}
    for d in range(2):
        for south_to_north in (True, False):
            path = tmp_path / f"date{d}" / ("s2n.grib" if south_to_north else "n2s.grib")
            path.parent.mkdir(exist_ok=True)
            path.write_bytes(ref.template_file(south_to_north))
            out[d, south_to_north] = path
    return out


def test_plane_reader_on_the_host(tmp_path):
    from py4cast_amd import grib2
    from py4cast_amd.diskio import GribPlaneReader

    files = _files(tmp_path)
    names = list(FIELD_OF)                                                 # surface types 103, 101 and 1 in one file
    want_lat = ref.LAT0 + np.arange(ref.NJ)[::-1] * ref.STEP               # north first
    results = {}
    for south_to_north in (True, False):
        reader = GribPlaneReader(device=None)
        selections = [[[(files[d, south_to_north], _fid(n)) for d in range(2)]] for n in names]            # F = 5, B = 1, T = 2
        planes, lat, lon = reader.read(selections)
        assert isinstance(planes, torch.Tensor) and planes.dtype == torch.float32 and tuple(planes.shape) == (len(names), 1, 2, ref.NJ, ref.NI)
        assert np.allclose(lat, want_lat, atol=1e-9) and np.allclose(lon, ref.LON0 - 360.0 + np.arange(ref.NI) * ref.STEP, atol=1e-9)
        messages = grib2.parse_messages(ref.template_file(south_to_north))
        for i, n in enumerate(names):
            for d in range(2):
                # row 0 is the northernmost row: a south-to-north stream is flipped, a north-to-south one is not
                assert cases.same_bits(planes[i, 0, d].numpy(), cases.expected_plane(messages[FIELD_OF[n]], flip=south_to_north)), (n, d)
        assert reader.parsed == 2
        reader.read(selections)
        assert reader.parsed == 2                                          # both files came out of the cache
        results[south_to_north] = planes
    # the builder writes the same values in stream order either way, so north-first planes of the two files mirror each other
    assert torch.equal(results[True], results[False].flip(-2))
    # the LRU keeps `cache` files: with room for one, alternating between two parses every time
    small = GribPlaneReader(device=None, cache=1)
    one = lambda d: [[[(files[d, True], _fid(names[0]))]]]   # noqa: E731
    for d in (0, 0, 1, 0, 0):
        small.read(one(d))
    assert small.parsed == 3 and list(small.files) == [str(files[0, True])]
    with pytest.raises(ValueError, match=r"selections\[F\]\[B\]\[T\]"):
        small.read([[[(files[0, True], _fid(names[0]))], []]])
    with pytest.raises(KeyError, match="no message"):
        small.read([[[(files[0, True], {"parameterCategory": 19})]]])


def test_plane_reader_refuses_mixed_grids(tmp_path):
    from py4cast_amd.diskio import GribPlaneReader

    g = np.random.default_rng(5)
    a, b = tmp_path / "a.grib", tmp_path / "b.grib"
    a.write_bytes(cases.random_message(g, 9, 5, 12, 0.0, 0, 0))
    b.write_bytes(cases.random_message(g, 9, 6, 12, 0.0, 0, 0))
    fid = {"parameterCategory": 0, "parameterNumber": 0}
    with pytest.raises(ValueError, match=r"b\.grib is on a grid of 6 x 9.*a\.grib on 5 x 9.*one call reads one grid"):
        GribPlaneReader(device=None).read([[[(a, fid), (b, fid)]]])
    # the same size at another place is another grid too: a south-to-north file of 5 rows and a north-to-south one cover the same
    # latitudes, one of 5 rows starting elsewhere does not
    c = tmp_path / "c.grib"
    c.write_bytes(cases.random_message(g, 9, 5, 12, 0.0, 0, 0, south_to_north=True))
    planes, lat, _ = GribPlaneReader(device=None).read([[[(a, fid), (c, fid)]]])
    assert tuple(planes.shape) == (1, 1, 2, 5, 9) and lat[0] > lat[-1]


def test_grib_batch_loader_validates_its_arguments(tmp_path):
    from py4cast_amd import diskio, regrid

    date = dt.datetime(2023, 1, 2, 3)
    assert diskio.titan_grib_path("/data/titan", "PAAROME_1S40_ECH0_2M.grib", date) == \
        diskio.Path("/data/titan/grib/2023-01-02_03h00/PAAROME_1S40_ECH0_2M.grib")
    plan = regrid.RegridPlan((ref.NJ, ref.NI), (ref.NJ, ref.NI))
    params = [("t2m", "a.grib", _fid("aro_t2m_2m"), "G"), ("u10", "a.grib", _fid("aro_u10_10m"), "G")]
    load = lambda **kw: diskio.load_titan_grib_batch(**{**dict(dataset_path=tmp_path, params=params, dates=[[date, date]], stats=None,   # noqa: E731
                                                               num_input_steps=1, forcing=None, plans={"G": plan}), **kw})
    with pytest.raises(ValueError, match="CUDA device"):
        load()
    with pytest.raises(ValueError, match="CUDA device"):
        load(reader=diskio.GribPlaneReader(device=None))
    with pytest.raises(ValueError, match="no parameters"):
        load(params=[])
    with pytest.raises(ValueError, match="no plan for the native grids \\['H'\\]"):
        load(params=params + [("r2", "a.grib", _fid("aro_r2_2m"), "H")])
    with pytest.raises(ValueError, match="appear twice"):
        load(params=params + [params[0]])
    with pytest.raises(ValueError, match="same, non-zero number of steps"):
        load(dates=[[date, date], [date]])
    with pytest.raises(ValueError, match="3 input steps of 2 dates"):
        load(num_input_steps=3)


def test_the_field_record_and_the_launch_constants_mirror_the_library():
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    handle = L.lib()
    assert (handle.p4c_grib_unpack_tile(), handle.p4c_grib_unpack_max_blocks()) == (ops.GRIB_UNPACK_TILE, ops.GRIB_UNPACK_MAX_BLOCKS)
    assert ops.GRIB_UNPACK_TILE % 32 == 0 and handle.p4c_grib_unpack_workspace_bytes(7) == 28
    assert ops.GRIB_FIELD.itemsize == 72 and [ops.GRIB_FIELD.fields[n][1] for n in ops.GRIB_FIELD.names] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56, 60, 64, 68]
    assert [handle.p4c_grib_unpack_fast(*a) for a in ((16, 0), (16, 1), (12, 0), (32, 0))] == [1, 0, 0, 0]
    table = ops.grib_fields([dict(stream_off=8, stream_len=10, ni=5, nj=1, count=5, nbits=16, R=1.5, E=-1, D=2)])
    assert table.dtype == ops.GRIB_FIELD and int(table[0]["bitmap_off"]) == -1 and float(table[0]["R"]) == 1.5
    with pytest.raises(L.P4CError, match="no column"):
        ops.grib_fields([dict(nbit=3)])
    with pytest.raises(L.P4CError):                                        # no CPU path
        ops.grib_unpack(torch.zeros(16, dtype=torch.uint8), table)
