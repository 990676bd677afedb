"""
The complex-packing route of the GRIB writer without a GPU: ``grib2.pack_complex`` (the contract of csrc/grib_pack_complex.hip in numpy)
byte for byte against bytes that never come from it (tests/grib_pack_complex_cases.py: the integers of tests/grib2_reference.py's float64
packer through the independent encoder of tests/grib_complex_cases.py in groups of 32, read back by its sequential decoder), ``encode``
with the complex arguments, the CPU writer's ``packing`` and the settings key.  tests/test_grib_pack_complex_gpu.py holds the device to
the same bytes.
"""
import datetime as dt
import json
import os
import struct
import sys
import types
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib2_reference as ref  # noqa: E402
import grib_complex_cases as cases  # noqa: E402
import grib_pack_complex_cases as pc  # noqa: E402

NAMES = ["aro_t2m_2m", "aro_u10_10m", "aro_z_500hpa", "aro_prmsl_0hpa", "aro_tp_0m", "aro_r2_2m"]     # the third one is not written
SIZES = [(1, 1), (1, 2), (1, 31), (1, 32), (1, 33), (37, 53)]


def _values(n, seed):
    g = np.random.default_rng(seed)
    x = np.arange(n, dtype=np.float64)
    return (280.0 + 6.0 * np.sin(x / 23.0) + 0.3 * g.standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def expected():
    """(order, (h, w), nbits) -> (v, expected_field(v)), computed once"""
    out = {}
    for order in (0, 1, 2):
        for h, w in SIZES:
            for nbits in (1, 12, 16, 24, pc.LIMITS[order]):
                v = _values(h * w, 100 * order + nbits + h)
                out[order, (h, w), nbits] = (v, pc.expected_field(v, 2, nbits, order))
    return out


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_complex_equals_the_independent_encoder(order, size, expected):
    """every number and every octet; the sequential decoder returns the integers of the float64 packer from the bytes under test"""
    from py4cast_amd import grib2

    h, w = size
    for nbits in (1, 12, 16, 24, pc.LIMITS[order]):
        v, (vmin, vmax, R, E, bad, X, numbers, payload) = expected[order, size, nbits]
        got = grib2.pack_complex(v, 2, nbits, order)
        assert (got[0], got[1], got[2], got[3], got[4]) == (vmin, vmax, R, E, 0) and bad == 0
        assert got[6] == payload, (nbits, len(got[6]), len(payload))
        for key in ("ival1", "ival2", "gmin", "ref_bits", "ng", "l_last"):
            assert got[5][key] == numbers[key], (key, nbits)
        assert len(payload) <= grib2.complex_capacity(h * w, nbits, order) == pc.capacity(h * w, nbits, order)
        msg = cases.assemble(w, h, cases.section5(h * w, float(R), E, 2, dict(numbers, **got[5])), got[6])
        assert cases.restate(msg)[0] == X


def test_one_step_past_a_limit_raises():
    from py4cast_amd import grib2

    v = _values(40, 1)
    for order, nbits in ((0, 33), (1, 31), (2, 30), (3, 8), (-1, 8), (0, 0)):
        with pytest.raises(grib2.GribError):
            grib2.pack_complex(v, 0, nbits, order)
        with pytest.raises(grib2.GribError):
            grib2.check_complex(nbits, order)
    for order in (0, 1, 2):
        grib2.pack_complex(v, 0, pc.LIMITS[order], order)


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 33, 37 * 53])
def test_a_constant_field_is_its_descriptors_and_its_widths(order, n):
    from py4cast_amd import grib2

    v = np.full(n, 281.25, dtype=np.float32)
    *_, numbers, payload = grib2.pack_complex(v, 2, 16, order)
    ng = -(-n // 32)
    assert numbers["ref_bits"] == 0 and len(payload) == (6 * ng + 7) // 8 + (4 * (order + 1) if order else 0)
    assert payload == pc.expected_field(v, 2, 16, order)[7]


@pytest.mark.parametrize("order", [0, 1, 2])
def test_the_group_widths_run_from_nothing_to_the_widest(order):
    """noise that grows along the stream: constant groups (width 0) up to groups that hold the extreme differences, whose width is
    nbits + order -- the most the capacity allows for"""
    from py4cast_amd import grib2

    nbits, n = 12, 4000
    v = pc.growing_noise(n, nbits)
    vmin, vmax, R, E, bad, numbers, payload = grib2.pack_complex(v, 0, nbits, order)
    *_, X, want, expected_payload = pc.expected_field(v, 0, nbits, order)
    assert payload == expected_payload
    ng = numbers["ng"]
    head = (4 * (order + 1) if order else 0) + (ng * numbers["ref_bits"] + 7) // 8
    bits = np.unpackbits(np.frombuffer(payload[head:head + (6 * ng + 7) // 8], dtype=np.uint8))[:6 * ng].reshape(ng, 6)
    widths = set((bits * (1 << np.arange(5, -1, -1))).sum(axis=1).tolist())
    assert {0, nbits + order} <= widths and max(widths) == nbits + order, sorted(widths)
    msg = cases.assemble(n, 1, cases.section5(n, float(R), E, 0, dict(want, **numbers)), payload)
    assert cases.restate(msg)[0] == X


def _template_message(data_template=0):
    from py4cast_amd import grib2

    return grib2.parse_messages(ref.template_file(south_to_north=True, data_template=data_template))[0]


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("window", [(0, ref.NJ - 1, 0, ref.NI - 1), (ref.ROW0, ref.ROW0 + ref.H - 1, ref.COL0, ref.COL0 + ref.W - 1)])
def test_encode_with_the_complex_arguments(order, window):
    """the 5.2 / 5.3 message of a field decodes -- by grib2.decode and by the sequential decoder -- to what its 5.0 message decodes to,
    bit for bit; the smaller window goes through the bitmap"""
    from py4cast_amd import grib2

    m = _template_message()
    r0, r1, c0, c1 = window
    count = (r1 - r0 + 1) * (c1 - c0 + 1)
    v = _values(count, 5)
    vmin, vmax, R, E, bad, stream = grib2.pack_simple(v, 2, 16)
    *_, numbers, payload = grib2.pack_complex(v, 2, 16, order)
    common = dict(window=window, R=float(R), E=E, D=2, nbits=16)
    simple = grib2.encode(m, ref.BASIS, dt.timedelta(hours=2), packed=stream, **common)
    msg = grib2.encode(m, ref.BASIS, dt.timedelta(hours=2), packed=payload, order=order, ref_bits=numbers["ref_bits"], **common)
    s5 = ref.walk(msg)[0][5]
    assert len(s5) == (49 if order else 47) and struct.unpack_from(">H", s5, 9)[0] == (3 if order else 2)
    want_s5 = cases.section5(count, float(R), E, 2, dict(order=order, nbytes=4 if order else 0, ng=numbers["ng"], ref_bits=numbers["ref_bits"],
                                                         w_ref=0, w_bits=6, l_ref=32, l_inc=1, l_last=numbers["l_last"], l_bits=0))
    assert s5 == want_s5
    want, keys = grib2.decode(simple)
    got, _ = grib2.decode(msg)
    assert np.array_equal(np.ma.getmaskarray(got), np.ma.getmaskarray(want))
    assert np.array_equal(got.filled(0.0).view(np.int64), want.filled(0.0).view(np.int64))
    plane = cases.restate(msg)[1]
    assert np.array_equal(np.isnan(plane), np.ma.getmaskarray(want))
    assert np.array_equal(plane[~np.isnan(plane)].view(np.int32), want.compressed().astype(np.float32).view(np.int32))
    # sections 0-4 and 6 do not depend on the packing
    a, b = ref.walk(simple)[0], ref.walk(msg)[0]
    assert all(a[i] == b[i] for i in (1, 3, 4, 6)) and a.get(2) == b.get(2)


def test_encode_without_the_new_arguments_returns_the_bytes_it_returned():
    """a fixed input: the length and the SHA-256 of the message as the code before the complex arguments wrote it; sections 5-7 are
    rebuilt from the layout as well"""
    from py4cast_amd import grib2

    m = _template_message()
    window = (ref.ROW0, ref.ROW0 + ref.H - 1, ref.COL0, ref.COL0 + ref.W - 1)
    v = _values(ref.H * ref.W, 9)
    vmin, vmax, R, E, bad, stream = grib2.pack_simple(v, 2, 16)
    assert stream == ref.pack(v, 2, 16)[5]
    msg = grib2.encode(m, ref.BASIS, dt.timedelta(hours=2), window=window, packed=stream, R=float(R), E=E, D=2, nbits=16)
    import hashlib

    assert len(msg) == 1307 and hashlib.sha256(msg).hexdigest() == "87c005df0e446cfa73d0b2e06925e65928f89f71f6fa530cae2e10f1998e5933"
    sections = ref.walk(msg)[0]
    assert sections[5] == ref.section5(ref.H * ref.W, float(R), E, 2, 16) and sections[7][5:] == stream
    present = np.zeros((ref.NJ, ref.NI), dtype=np.uint8)
    present[window[0]:window[1] + 1, window[2]:window[3] + 1] = 1
    assert sections[6] == struct.pack(">IBB", 6 + ref.NJ * ref.NI // 8, 6, 0) + np.packbits(present.reshape(-1)).tobytes()
    assert len(msg) == 16 + sum(len(sections[i]) for i in (1, 3, 4, 5, 6, 7)) + 4
    with pytest.raises(grib2.GribError):
        grib2.encode(m, ref.BASIS, dt.timedelta(hours=2), window=window, packed=stream[:-1], R=float(R), E=E, D=2, nbits=16)
    with pytest.raises(grib2.GribError):      # a payload shorter than its descriptors and tables
        grib2.encode(m, ref.BASIS, dt.timedelta(hours=2), window=window, packed=b"\x00" * 8, R=float(R), E=E, D=2, nbits=16, order=2)


# ------------------------------------------------------------------------------------------------ the writer
def mixed_template(south_to_north=True, order_octet=None, short=None):
    """ref.template_file with message 1 (u10) re-packed in 5.2, message 3 (r2) in 5.3 at order 1 and message 4 (pmer) in 5.3 at order 2
    by the independent encoder, the others in 5.0.  order_octet: what octet 48 of message 4 says; short: the message whose section 5
    says template 5.3 in 21 octets"""
    out, at = [], 0
    data = ref.template_file(south_to_north=south_to_north)
    for i, sections in enumerate(ref.walk(data)):
        total = struct.unpack_from(">Q", sections[0], 8)[0]
        msg = data[at:at + total]
        at += total
        order = {1: 0, 3: 1, 4: 2}.get(i)
        if i == short:
            msg = cases.patched(msg, 5, lambda s: s.__setitem__(slice(9, 11), struct.pack(">H", 3)))
        elif order is not None:
            k = ref.keys(sections)
            X = pc.integers(sections[7][5:], k["count"], k["nbits"])
            numbers, payload, _ = cases.encode(X, order, range(0, len(X), 40), nbytes=4 if order else 0, ref_bits=k["nbits"])
            msg = cases.patched(msg, 5, lambda s, n=numbers, k=k: bytearray(cases.section5(k["count"], k["R"], k["E"], k["D"], n)))
            msg = cases.patched(msg, 7, lambda s, p=payload: bytearray(s[:5]) + p)
            if i == 4 and order_octet is not None:
                msg = cases.patched(msg, 5, lambda s: s.__setitem__(47, order_octet))
        out.append(msg)
    return b"".join(out)


def _settings(root, **extra):
    from py4cast_amd.outputs import OutputSavingSettings

    (root / "gribs").mkdir(parents=True, exist_ok=True)
    io = root / "io.json"
    io.write_text(json.dumps(dict({"template_grib": "../template.grib", "path_to_runtime": "{}", "dir_grib": str(root / "gribs"),
                                   "dir_gif": str(root / "gifs"), "grib_fmt": "mb{}_ech_{}.grib", "grib_identifiers": ["member", "leadtime"]},
                                  **extra)))
    return OutputSavingSettings.from_json(io)


def _prediction():
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(2, 2, ref.H, ref.W, len(NAMES), generator=g)
    return pred, torch.tensor([6.0, 4.0, 80.0, 900.0, 1.5, 20.0]), torch.tensor([283.0, -1.0, 5500.0, 101300.0, 2.0, 60.0])


def _samples():
    from py4cast_amd.outputs import GribSample

    out = []
    for b in range(2):
        start = dt.datetime(2023, 1, 1, 6 * b)
        deltas = [dt.timedelta(hours=i - 1) for i in range(4)]
        sample = types.SimpleNamespace(timestamps=types.SimpleNamespace(datetime=start, timedeltas=deltas), member=b,
                                       output_timestamps=types.SimpleNamespace(datetime=start, timedeltas=deltas[2:]))
        out.append(GribSample.from_sample(sample, start.strftime("%Y%m%d%H")))
    return out


def _write(root, template_bytes, **kwargs):
    """the files of one batch through the CPU writer -> {relative path: bytes}, the writer"""
    from py4cast_amd.namedtensor import NamedTensor
    from py4cast_amd.outputs import ForecastGribWriter

    root.mkdir(parents=True, exist_ok=True)
    (root / "template.grib").write_bytes(template_bytes)
    lat, lon = ref.forecast_grid()
    writer = ForecastGribWriter(_settings(root), torch.device("cpu"), lat, lon, **kwargs)
    pred, std, mean = _prediction()
    writer.submit(NamedTensor(pred, ["batch", "timestep", "lat", "lon", "features"], list(NAMES)), std, mean, _samples())
    writer.drain()
    assert len(writer.written) == 4 and not writer._pending
    return {str(p.relative_to(root)): p for p in writer.written}, writer


def _planes(paths):
    """every written plane through GribPlaneReader on the CPU: {(file, message index): (Nj, Ni) fp32}"""
    from py4cast_amd import grib2
    from py4cast_amd.diskio import GribPlaneReader
    from py4cast_amd.outputs import grib_fid

    reader = GribPlaneReader(device=None)
    out = {}
    for rel, path in paths.items():
        for name in NAMES:
            fid = grib_fid(name, 3600)[0]
            if fid is None:
                continue
            fid = {k: v for k, v in fid.items() if k in grib2.MATCHED_KEYS}
            planes, lat, lon = reader.read([[[(path, fid)]]])
            out[rel, name] = planes[0, 0, 0].numpy().copy()
    return out


@pytest.mark.parametrize("south_to_north", [True, False])
def test_the_cpu_writer_follows_the_template(tmp_path, south_to_north):
    """a template file with 5.0, 5.2 and 5.3 messages: each feature in its message's packing; the window is smaller than the template
    grid (bitmap); GribPlaneReader reads every plane back equal, bit for bit, to the one read from the "simple" files; the integers of
    every complex message are those of the float64 packer"""
    from py4cast_amd import grib2

    template = mixed_template(south_to_north)
    simple, _ = _write(tmp_path / "simple", template)
    followed, _ = _write(tmp_path / "template", template, packing="template")
    complex_, _ = _write(tmp_path / "complex", template, packing="complex")
    assert sorted(simple) == sorted(followed) == sorted(complex_)
    for rel in simple:
        numbers = lambda paths: [m.keys["dataRepresentationTemplateNumber"] for m in grib2.read_messages(paths[rel])]   # noqa: E731
        assert numbers(simple) == [0] * 5 and numbers(followed) == [0, 2, 3, 0, 3] and numbers(complex_) == [3] * 5
        orders = [m.sections[5][47] if len(m.sections[5]) == 49 else None for m in grib2.read_messages(followed[rel])]
        assert orders == [None, None, 2, None, 1]                  # t2m, u10, pmer, tp, r2
        assert all(m.sections[5][47] == 2 and m.keys["bitMapIndicator"] == 0 for m in grib2.read_messages(complex_[rel]))
        # the 5.0 messages of "template" are the bytes of "simple"
        a, b = grib2.read_messages(simple[rel]), grib2.read_messages(followed[rel])
        assert a[0].raw == b[0].raw and a[3].raw == b[3].raw and a[1].raw != b[1].raw
        for s, c in zip(a, grib2.read_messages(complex_[rel])):       # the integers, by the sequential decoder
            k = ref.keys(ref.walk(s.raw)[0])
            assert cases.restate(c.raw)[0] == pc.integers(s.sections[7][5:], k["count"], k["nbits"])
    want = _planes(simple)
    for other in (followed, complex_):
        got = _planes(other)
        assert sorted(got) == sorted(want) and len(want) == 20
        for key, plane in want.items():
            assert plane.shape == (ref.NJ, ref.NI) and np.isnan(plane).sum() == ref.NJ * ref.NI - ref.H * ref.W
            assert np.array_equal(plane.view(np.int32), got[key].view(np.int32)), key


def test_the_default_writer_writes_the_bytes_of_a_writer_without_the_argument(tmp_path):
    template = mixed_template()
    a, writer = _write(tmp_path / "a", template)
    b, _ = _write(tmp_path / "b", template, packing="simple")
    assert writer.packing == "simple"
    assert {k: p.read_bytes() for k, p in a.items()} == {k: p.read_bytes() for k, p in b.items()}
    # and they are the simple-packed messages of the restatement's packer
    pred, std, mean = _prediction()
    for rel, path in a.items():
        for sections in ref.walk(path.read_bytes()):
            assert ref.keys(sections)["data_template"] == 0 and len(sections[5]) == 21


def test_a_template_the_writer_cannot_follow_raises_with_the_octet(tmp_path):
    from py4cast_amd import grib2

    with pytest.raises(grib2.GribError, match="section 5 octet 48"):
        _write(tmp_path / "order3", mixed_template(order_octet=3), packing="template")
    with pytest.raises(grib2.GribError, match="section 5 octets 1-4"):
        _write(tmp_path / "short", mixed_template(short=0), packing="template")
    with pytest.raises(ValueError, match="packing"):
        _write(tmp_path / "name", mixed_template(), packing="jpeg")
    # the same templates are fine for the default writer, which only takes D and nbits from them
    _write(tmp_path / "order3_simple", mixed_template(order_octet=3))


def test_a_width_past_the_limits_falls_back_to_simple_packing_with_one_warning(tmp_path):
    """nbits = 30 in the template of t2m: order 2 does not take it"""
    from py4cast_amd import grib2

    data = ref.template_file(south_to_north=True)
    first = struct.unpack_from(">Q", data, 8)[0]
    wide = cases.patched(data[:first], 5, lambda s: s.__setitem__(19, 30)) + data[first:]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        paths, _ = _write(tmp_path / "wide", wide, packing="complex")
    assert len([w for w in caught if "simple packing" in str(w.message)]) == 1
    for path in paths.values():
        assert [m.keys["dataRepresentationTemplateNumber"] for m in grib2.read_messages(path)] == [0, 3, 3, 3, 3]


def test_the_settings_file_with_and_without_grib_packing(tmp_path):
    from py4cast_amd.outputs import ForecastGribWriter

    assert _settings(tmp_path / "a").grib_packing == "simple"
    settings = _settings(tmp_path / "b", grib_packing="template")
    assert settings.grib_packing == "template"
    (tmp_path / "b" / "template.grib").write_bytes(mixed_template())
    lat, lon = ref.forecast_grid()
    ds = types.SimpleNamespace(sample_list=[], grid=types.SimpleNamespace(lat=lat, lon=lon))
    assert ForecastGribWriter.for_dataset(settings, ds, torch.device("cpu")).packing == "template"
    with pytest.raises(TypeError):
        _settings(tmp_path / "c", grib_compression="jpeg")
