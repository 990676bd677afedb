"""
GRIB2 on a regular latitude / longitude grid, restated for the tests (test infrastructure, never product code; not collected).

Written from the WMO layout (FM 92 GRIB edition 2: sections 0-8, grid definition template 3.0, product definition templates 4.0 and
4.8, data representation template 5.0), NOT from py4cast_amd/grib2.py: a ``struct``-level builder of template files, a section walker
and decoder that work on 0-based offsets, and the float64 packer of the contract of csrc/grib_pack.hip with ``np.nextafter`` on
binary32 for R, exact rational arithmetic for E and Python integers for the bit stream.

The contract, one field (values v in stream order, decimal scale factor D, width nbits):
  v = fp32(fp32(x * std) + mean);  vmin / vmax over the finite v ((NaN, NaN) without one);  bad = how many v are not finite;
  s(v) = v * 10^D (D >= 0) or v / 10^-D, in float64;   R = the largest binary32 <= s(vmin);
  E = the smallest integer with (s(vmax) - R) / 2^E <= 2^nbits - 1, 0 when vmax == vmin;
  X = min(floor((s(v) - R) / 2^E + 0.5), 2^nbits - 1);  the stream holds X in nbits bits each, most significant bit first, zero-padded.
"""
import datetime as dt
import math
import struct
from fractions import Fraction

import numpy as np

NJ, NI = 24, 40                       # the template grids
LAT0, LON0, STEP = -2.0, 355.0, 0.025  # southern latitudes (sign and magnitude), longitudes stored as 355 .. 356: -5 .. -4 after the wrap
ROW0, COL0 = 2, 5                     # where the 18 x 28 forecast grid sits in the south-to-north template
H, W = 18, 28
BASIS = dt.datetime(2021, 3, 4, 5, 0, 0)


def sm(value, n):
    """sign-and-magnitude, n octets"""
    raw = abs(int(value)) | ((1 << (8 * n - 1)) if value < 0 else 0)
    return raw.to_bytes(n, "big")


def unsm(raw):
    value = int.from_bytes(raw, "big")
    top = 1 << (8 * len(raw) - 1)
    return -(value - top) if value >= top else value


# ------------------------------------------------------------------------------------------------ the packer
def pack(v, D, nbits):
    """-> (vmin, vmax, R as np.float32, E, bad, stream bytes or None when bad > 0)"""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    finite = np.isfinite(v)
    bad = int((~finite).sum())
    p = float(10 ** abs(D))                                # an integer below 2^53: exact
    if bad == v.size:
        return np.float32(np.nan), np.float32(np.nan), np.float32(0), 0, bad, None
    vmin, vmax = np.float32(v[finite].min()), np.float32(v[finite].max())
    scaled = (lambda x: np.float64(x) * p) if D >= 0 else (lambda x: np.float64(x) / p)
    smin, smax = scaled(vmin), scaled(vmax)
    R = np.float32(smin)
    while np.float64(R) > smin:
        R = np.nextafter(R, np.float32(-np.inf))
    assert np.float64(R) <= smin < np.float64(np.nextafter(R, np.float32(np.inf)))
    top = 2 ** nbits - 1
    E = 0
    if vmax != vmin:
        span = Fraction(float(smax - np.float64(R)))        # the rounded float64 difference, then exact
        E = math.ceil(math.log2(float(span) / top))
        while span / Fraction(2) ** E > top:
            E += 1
        while span / Fraction(2) ** (E - 1) <= top:
            E -= 1
    if bad:
        return vmin, vmax, R, E, bad, None
    X = np.minimum(np.floor(np.ldexp(scaled(v) - np.float64(R), -E) + 0.5), float(top))
    X = [int(x) for x in X] + [0] * (-v.size % 8)
    out = bytearray()
    for g in range(0, len(X), 8):                          # 8 values are nbits whole octets
        word = 0
        for x in X[g:g + 8]:
            word = (word << nbits) | x
        out += word.to_bytes(nbits, "big")
    return vmin, vmax, R, E, bad, bytes(out[:(v.size * nbits + 7) // 8])


def expected(pred, std, mean, spec, samples, features, h, w, flip):
    """pred (B,T,N,F) float32 numpy -> params (n,T,K,5) int32 and streams[(i,t,k)] = bytes or None"""
    pred, std, mean = (np.asarray(a, dtype=np.float32) for a in (pred, std, mean))
    n, T, K = len(samples), pred.shape[1], len(features)
    params, streams = np.zeros((n, T, K, 5), dtype=np.int32), {}
    for i, b in enumerate(samples):
        for t in range(T):
            for k, f in enumerate(features):
                a = (pred[b, t, :, f] * std[f]).astype(np.float32)
                v = (a + mean[f]).astype(np.float32).reshape(h, w)
                v = v[::-1] if flip else v
                vmin, vmax, R, E, bad, stream = pack(v, *spec[k])
                params[i, t, k, :3] = np.array([vmin, vmax, R], dtype=np.float32).view(np.int32)
                params[i, t, k, 3:] = (E, bad)
                streams[i, t, k] = stream
    return params, streams


# ------------------------------------------------------------------------------------------------ the data cases of the GPU test
#        B  T   H    W   F  samples  features               spec (D, nbits) per packed feature                    flip
SHAPES = {
    "gather": (2, 2, 18, 28, 21, None, (0, 3, 7, 8, 15, 20), [(2, 16), (0, 12), (-1, 16), (2, 8), (0, 11), (2, 24)], False),
    "dense": (2, 2, 18, 28, 8, (1,), (0, 1, 2, 4, 5, 7), [(0, 32), (2, 16), (-1, 24), (2, 12), (0, 8), (2, 11)], True),
    "tail_dense": (1, 1, 5, 7, 3, None, (0, 1, 2), [(2, 16), (0, 11), (-1, 12)], True),
    "tail_gather": (1, 2, 5, 7, 8, None, (6, 1), [(0, 11), (2, 24)], False),
}
LOOP = {"dense": (2, 2, 33, 997, 4, None, (0, 2, 3), [(2, 16), (0, 11), (-1, 8)], True),
        "gather": (2, 2, 33, 997, 9, None, (8, 1), [(2, 16), (0, 11)], False)}


def case(shape, seed=0):
    B, T, h, w, F, samples, features, spec, flip = shape
    g = np.random.default_rng(seed)
    pred = g.standard_normal((B, T, h * w, F)).astype(np.float32)
    std = (0.5 + 4.0 * g.random(F)).astype(np.float32)
    mean = (g.standard_normal(F) * 20.0).astype(np.float32)
    mean[features[0]] = np.float32(281.3)
    if len(features) > 3:
        pred[:, T - 1, :, features[3]] = np.float32(0.37)           # a constant field, in every sample
        pred[B - 1, 0, (h * w) // 3, features[2]] = np.nan           # one NaN: this field alone is reported
    samples = tuple(range(B)) if samples is None else samples
    return dict(pred=pred.reshape(B, T, h, w, F), std=std, mean=mean, spec=spec, samples=samples, features=features, H=h, W=w, flip=flip)


def expected_of(c):
    B, T, h, w, F = c["pred"].shape
    return expected(c["pred"].reshape(B, T, h * w, F), c["std"], c["mean"], c["spec"], c["samples"], c["features"], h, w, c["flip"])


# ------------------------------------------------------------------------------------------------ the builder
def section1(when):
    return struct.pack(">IBHHBBBHBBBBBBB", 21, 1, 85, 0, 15, 1, 1, when.year, when.month, when.day, when.hour, when.minute, when.second, 0, 1)


def section3(south_to_north, scan_extra=0, template=0, ni=NI, nj=NJ):
    micro = lambda x: int(round(x * 1e6))  # noqa: E731
    la_s, la_n = micro(LAT0), micro(LAT0 + (nj - 1) * STEP)
    la1, la2 = (la_s, la_n) if south_to_north else (la_n, la_s)
    lo1, lo2 = micro(LON0), micro(LON0 + (ni - 1) * STEP)
    scan = (0x40 if south_to_north else 0) | scan_extra
    body = (struct.pack(">BIBBH", 0, ni * nj, 0, 0, template) + bytes([6]) + b"\xff" * 15 + struct.pack(">IIII", ni, nj, 0, 0xFFFFFFFF)
            + sm(la1, 4) + sm(lo1, 4) + bytes([0x30]) + sm(la2, 4) + sm(lo2, 4) + struct.pack(">IIB", micro(STEP), micro(STEP), scan))
    return struct.pack(">IB", 5 + len(body), 3) + body


def section4(category, number, surface, level, template=0, unit=1, forecast=1, end=None, length=1, process=1, coordinates=0):
    """level: None = missing scale factor and value; (scale, value) otherwise"""
    first = b"\xff" * 5 if level is None else sm(level[0], 1) + sm(level[1], 4)
    body = (struct.pack(">HHBBBBBHBBI", coordinates, template, category, number, 2, 0, 0, 0, 0, unit, forecast) + bytes([surface]) + first
            + bytes([255]) + b"\xff" * 5)
    if template == 8:
        body += struct.pack(">HBBBBBBIBBBIBI", end.year, end.month, end.day, end.hour, end.minute, end.second, 1, 0, process, 2, 1, length, 255, 0)
    return struct.pack(">IB", 5 + len(body), 4) + body


def section5(count, R, E, D, nbits, template=0):
    return struct.pack(">IBIH", 21, 5, count, template) + struct.pack(">f", R) + sm(E, 2) + sm(D, 2) + bytes([nbits, 0])


def message(discipline, s1, s3, s4, values, D, nbits, local=None, data_template=0):
    """a whole message around ``values`` (all points present, stream order)"""
    _, _, R, E, _, stream = pack(values, D, nbits)
    parts = [s1] + ([struct.pack(">IB", 5 + len(local), 2) + local] if local is not None else [])
    parts += [s3, s4, section5(np.asarray(values).size, R, E, D, nbits, data_template), struct.pack(">IBB", 6, 6, 255),
              struct.pack(">IB", 5 + len(stream), 7) + stream, b"7777"]
    return b"GRIB\x00\x00" + bytes([discipline, 2]) + struct.pack(">Q", 16 + sum(len(p) for p in parts)) + b"".join(parts)


LOCAL = b"local use \x00\x01\x02 bytes"
#           name          category number surface level         D  nbits template
FIELDS = [("temperature", 0, 0, 103, (1, 20), 2, 16, 0),        # level 2 m as 20 with scale factor 1
          ("u10", 2, 2, 103, (0, 10), 0, 12, 0),
          ("v10", 2, 3, 103, (0, 10), 2, 16, 0),
          ("r2", 1, 1, 103, (0, 2), 0, 12, 0),
          ("pmer", 3, 1, 101, None, -1, 16, 0),
          ("tp", 1, 65, 1, None, 2, 16, 8)]


def template_file(south_to_north=True, scan_extra=0, grid_template=0, coordinates=0, data_template=0):
    """the bytes of a template file: one message per entry of FIELDS, the second with a section 2"""
    g = np.random.default_rng(11)
    out = []
    for i, (name, category, number, surface, level, D, nbits, pdt) in enumerate(FIELDS):
        values = (g.standard_normal(NJ * NI) * 3.0 + 10.0 * i).astype(np.float32)
        s4 = section4(category, number, surface, level, template=pdt, end=dt.datetime(2020, 1, 1, 1), coordinates=coordinates)
        out.append(message(0, section1(dt.datetime(2020, 1, 1, 0)), section3(south_to_north, scan_extra, grid_template), s4, values, D, nbits,
                           local=LOCAL if i == 1 else None, data_template=data_template))
    return b"".join(out)


def forecast_grid():
    """(lat (H,W), lon (H,W)) of the forecast grid: row 0 the southern one, inside the template's grid"""
    lat = LAT0 + (ROW0 + np.arange(H)) * STEP
    lon = (LON0 - 360.0) + (COL0 + np.arange(W)) * STEP
    return np.repeat(lat[:, None], W, axis=1), np.repeat(lon[None, :], H, axis=0)


# ------------------------------------------------------------------------------------------------ the walker and decoder
def walk(data):
    """-> a list of messages, each {section number: bytes}; total length and the end marker are checked"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"GRIB" and data[at + 7] == 2, "no edition-2 indicator section"
        total = struct.unpack_from(">Q", data, at + 8)[0]
        raw = data[at:at + total]
        assert len(raw) == total and raw[-4:] == b"7777", "total length / 7777"
        sections, pos = {0: raw[:16]}, 16
        while pos < total - 4:
            length, number = struct.unpack_from(">IB", raw, pos)
            assert number not in sections and pos + length <= total - 4
            sections[number] = raw[pos:pos + length]
            pos += length
        assert pos == total - 4
        out.append(sections)
        at += total
    return out


def keys(sections):
    s1, s3, s4, s5 = sections[1], sections[3], sections[4], sections[5]
    k = {"discipline": sections[0][6], "reference": dt.datetime(struct.unpack_from(">H", s1, 12)[0], *s1[14:19]),
         "category": s4[9], "number": s4[10], "template": struct.unpack_from(">H", s4, 7)[0], "unit": s4[17],
         "forecast": struct.unpack_from(">I", s4, 18)[0], "surface": s4[22], "ni": struct.unpack_from(">I", s3, 30)[0],
         "nj": struct.unpack_from(">I", s3, 34)[0], "scan": s3[71], "count": struct.unpack_from(">I", s5, 5)[0],
         "data_template": struct.unpack_from(">H", s5, 9)[0], "R": struct.unpack_from(">f", s5, 11)[0], "E": unsm(s5[15:17]),
         "D": unsm(s5[17:19]), "nbits": s5[19], "bitmap": sections[6][5], "local": sections.get(2, b"")[5:] if 2 in sections else None}
    if k["template"] == 8:
        k.update(end=dt.datetime(struct.unpack_from(">H", s4, 34)[0], *s4[36:41]), ranges=s4[41], process=s4[46], length_unit=s4[48],
                 length=struct.unpack_from(">I", s4, 49)[0])
    return k


def decode(sections):
    """-> ((nj, ni) float64 values in stream order, (nj, ni) bool present)"""
    k = keys(sections)
    assert k["data_template"] == 0
    points = k["ni"] * k["nj"]
    if k["bitmap"] == 255:
        present = [True] * points
    else:
        bits = int.from_bytes(sections[6][6:], "big")
        width = 8 * len(sections[6][6:])
        present = [bool((bits >> (width - 1 - i)) & 1) for i in range(points)]
    assert sum(present) == k["count"]
    data = sections[7][5:]
    assert len(data) == (k["count"] * k["nbits"] + 7) // 8
    stream, width = int.from_bytes(data, "big"), 8 * len(data)
    X = [(stream >> (width - (i + 1) * k["nbits"])) & ((1 << k["nbits"]) - 1) for i in range(k["count"])]
    values = np.zeros(points)
    values[np.array(present)] = [(Fraction(float(k["R"])) + x * Fraction(2) ** k["E"]) / Fraction(10) ** k["D"] for x in X]
    return values.reshape(k["nj"], k["ni"]), np.array(present).reshape(k["nj"], k["ni"])
