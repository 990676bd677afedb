"""
What the tests of the complex-packing decode (GRIB2 templates 5.2 / 5.3) need (test infrastructure, never product code; not collected):
an encoder from a GIVEN int64 field f to a whole message with every parameter of the templates in the caller's hand, a sequential
restatement of the decode in plain loops over Python integers, and the layout of a batch of such fields in one byte buffer for
``ops.grib_unpack_complex``.  Written from the WMO layout as g2clib's ``comunpack`` reads it, NOT from py4cast_amd/grib2.py.

The expected planes everywhere come from the integers handed to the encoder: ``float32((R + ldexp(float64(f), E)) / 10^D)`` (``*
10^-D`` for D < 0), NaN at absent points -- never from the code under test.  That is the decode's contract, a sequence of single
rounded float64 operations, so the comparison is bit for bit (``same_bits``), NaNs by position.
"""
import datetime as dt
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib2_reference as ref  # noqa: E402
from grib_unpack_cases import GUARD, SENTINEL, expected_buffer, same_bits, window_present  # noqa: E402,F401
from grib_unpack_cases import message as simple_message  # noqa: E402

MASK64 = (1 << 64) - 1


def _put(bits, starts, values, width):
    """write the ``width``-bit integers ``values`` at the bit positions ``starts`` of the 0/1 array ``bits``, most significant first"""
    if width == 0 or len(values) == 0:
        return
    values = np.asarray(values, dtype=np.uint64)
    idx = np.asarray(starts, dtype=np.int64)[:, None] + np.arange(width, dtype=np.int64)
    bits[idx] = ((values[:, None] >> np.arange(width - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)


def encode(f, order, bounds, *, nbytes=2, ref_bits=16, w_ref=0, w_bits=6, l_ref=0, l_inc=1, l_bits=8, widths=None, gmin=None,
           placeholder=0, last_stored=None):
    """The section-5 tail and the section-7 payload of the int64 field ``f`` (one value per packed point, stream order).

    order: 0 (template 5.2), 1 or 2 (5.3).  bounds: the first value of every group, ascending, bounds[0] == 0; two equal bounds make
    a group of length 0; the last group ends at len(f).  The reference of a group is the minimum of its X (0 with ref_bits == 0), its
    width the bits of the largest remainder but at least w_ref -- or widths[g] -- and gmin the minimum of the differences -- or the
    given one.  X[:order] = placeholder.  last_stored: the scaled length stored for the last group (default: its true one if that can
    be stored, else 0); its true length goes to octets 43-46.  Asserts that the parameters can represent the field.
    -> (dict of the template's numbers, payload bytes, X as a list of Python integers)."""
    f = [int(v) for v in np.asarray(f).reshape(-1)]
    n = len(f)
    bounds = [int(b) for b in bounds]
    ng = len(bounds)
    assert (ng == 0 and n == 0) or (ng > 0 and bounds[0] == 0 and all(a <= b for a, b in zip(bounds, bounds[1:])) and bounds[-1] <= n)
    if order == 0:
        ival1 = ival2 = g_min = 0
        X = list(f)
    else:
        if order == 1:
            d = [f[k] - f[k - 1] for k in range(1, n)]
        else:
            d = [f[k] - 2 * f[k - 1] + f[k - 2] for k in range(2, n)]
        g_min = (min(d) if d else 0) if gmin is None else int(gmin)
        X = [int(placeholder)] * min(order, n) + [v - g_min for v in d]
        ival1 = f[0] if n > 0 else 0
        ival2 = f[1] if n > 1 and order == 2 else 0
        if nbytes == 0:
            assert ival1 == 0 and ival2 == 0 and g_min == 0, "descriptors of no octets are 0"
        else:
            assert max(abs(ival1), abs(ival2), abs(g_min)) < 1 << (8 * nbytes - 1), "a descriptor does not fit nbytes octets"
    assert all(v >= 0 for v in X), "X must not be negative"
    ends = bounds[1:] + [n]
    lengths = [e - b for b, e in zip(bounds, ends)]
    refs, wds = [], []
    for g, (b, e) in enumerate(zip(bounds, ends)):
        r = min(X[b:e]) if e > b and ref_bits > 0 else 0
        need = max((v - r).bit_length() for v in X[b:e]) if e > b else 0
        w = max(need, w_ref) if widths is None else int(widths[g])
        assert need <= w <= 32 and 0 <= w - w_ref < max(1 << w_bits, 1) and r < max(1 << ref_bits, 1), (g, r, need, w)
        refs.append(r)
        wds.append(w)
    scaled = []
    for g, ln in enumerate(lengths):
        last = g == ng - 1
        fits = ln >= l_ref and (ln == l_ref or (l_inc > 0 and (ln - l_ref) % l_inc == 0)) and \
            (0 if ln == l_ref else (ln - l_ref) // l_inc) < max(1 << l_bits, 1)
        assert last or fits, f"group {g}: a length of {ln} is not l_ref + l_inc * (a {l_bits}-bit number)"
        own = (0 if ln == l_ref else (ln - l_ref) // l_inc) if fits else 0
        scaled.append(int(last_stored) if last and last_stored is not None else own)
    assert all(0 <= s < max(1 << l_bits, 1) for s in scaled)
    descriptors = b""
    if order:
        for v in ([ival1, ival2, g_min] if order == 2 else [ival1, g_min]):
            descriptors += ref.sm(v, nbytes) if nbytes else b""
    pad8 = lambda b: (b + 7) // 8 * 8   # noqa: E731
    at_ref = 8 * len(descriptors)
    at_w = at_ref + pad8(ng * ref_bits)
    at_l = at_w + pad8(ng * w_bits)
    at_v = at_l + pad8(ng * l_bits)
    value_bits = sum(ln * w for ln, w in zip(lengths, wds))
    bits = np.zeros(pad8(at_v + value_bits), dtype=np.uint8)
    bits[:at_ref] = np.unpackbits(np.frombuffer(descriptors, dtype=np.uint8))
    g = np.arange(ng, dtype=np.int64)
    _put(bits, at_ref + g * ref_bits, refs, ref_bits)
    _put(bits, at_w + g * w_bits, [w - w_ref for w in wds], w_bits)
    _put(bits, at_l + g * l_bits, scaled, l_bits)
    if n:
        group = np.repeat(g, lengths)
        wd = np.asarray(wds, dtype=np.int64)
        ln = np.asarray(lengths, dtype=np.int64)
        first = np.cumsum(ln) - ln
        first_bit = at_v + np.cumsum(ln * wd) - ln * wd
        k = np.arange(n, dtype=np.int64)
        start = first_bit[group] + (k - first[group]) * wd[group]
        rest = np.array([X[i] - refs[group[i]] for i in range(n)], dtype=np.uint64)
        for w in set(wds):
            mine = wd[group] == w
            _put(bits, start[mine], rest[mine], w)
    numbers = dict(order=order, nbytes=nbytes if order else 0, ng=ng, ref_bits=ref_bits, w_ref=w_ref, w_bits=w_bits, l_ref=l_ref, l_inc=l_inc,
                   l_last=lengths[-1] if ng else 0, l_bits=l_bits, ival1=ival1, ival2=ival2, gmin=g_min)
    return numbers, np.packbits(bits).tobytes(), X


def section5(count, R, E, D, numbers):
    """template 5.2 (47 octets) or 5.3 (49)"""
    t = numbers
    body = (struct.pack(">IH", count, 3 if t["order"] else 2) + struct.pack(">f", R) + ref.sm(E, 2) + ref.sm(D, 2)
            + bytes([t["ref_bits"], 0, 1, 0]) + bytes(8) + struct.pack(">IBBIBIB", t["ng"], t["w_ref"], t["w_bits"], t["l_ref"], t["l_inc"],
                                                                     t["l_last"], t["l_bits"]))
    if t["order"]:
        body += bytes([t["order"], t["nbytes"]])
    return struct.pack(">IB", 5 + len(body), 5) + body


def assemble(ni, nj, s5, payload, present=None, south_to_north=False, category=0, number=0):
    """a whole message on an nj x ni grid around a section 5 and a section-7 payload"""
    if present is None:
        s6 = struct.pack(">IBB", 6, 6, 255)
    else:
        bitmap = np.packbits(np.asarray(present, dtype=np.uint8).reshape(-1)).tobytes()
        s6 = struct.pack(">IBB", 6 + len(bitmap), 6, 0) + bitmap
    parts = [ref.section1(dt.datetime(2020, 1, 1, 0)), ref.section3(south_to_north, ni=ni, nj=nj), ref.section4(category, number, 103, (0, 2)),
             s5, s6, struct.pack(">IB", 5 + len(payload), 7) + payload, b"7777"]
    return b"GRIB\x00\x00" + bytes([0, 2]) + struct.pack(">Q", 16 + sum(len(p) for p in parts)) + b"".join(parts)


def message(ni, nj, f, order, bounds, R, E, D, present=None, south_to_north=False, count=None, category=0, number=0, **params):
    """A whole message around the integers f (one per PRESENT point, stream order); count: what section 5 says (default len(f));
    params: those of ``encode``."""
    f = np.asarray(f).reshape(-1)
    assert f.size == (ni * nj if present is None else int(np.count_nonzero(present)))
    numbers, payload, _ = encode(f, order, bounds, **params)
    return assemble(ni, nj, section5(f.size if count is None else count, R, E, D, numbers), payload, present, south_to_north, category, number)


def patched(msg, number, change):
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


def random_bounds(g, n, lo=1, hi=40):
    """group starts for n values with lengths uniform in lo .. hi"""
    bounds, at = [], 0
    while at < n:
        bounds.append(at)
        at += int(g.integers(lo, hi + 1))
    return bounds


def smooth_field(g, n, amplitude=2000, noise=6, offset=0):
    """an int64 field of n values that complex packing suits: a slow wave plus a little noise"""
    x = np.arange(n, dtype=np.float64)
    return (offset + amplitude * np.sin(x / 37.0) + g.integers(-noise, noise + 1, size=n)).astype(np.int64)


def expected_plane(f, ni, nj, R, E, D, present=None, flip=False, count=None):
    """(nj, ni) float32 from the integers handed to the encoder: the k-th present point takes f[k] for k < count"""
    f = np.asarray(f, dtype=np.int64).reshape(-1)
    count = f.size if count is None else count
    where = np.arange(ni * nj) if present is None else np.flatnonzero(np.asarray(present).reshape(-1))
    n = min(count, where.size, f.size)
    with np.errstate(all="ignore"):
        t = np.float64(np.float32(R)) + np.ldexp(f[:n].astype(np.float64), E)
        y = t / np.float64(10 ** D) if D >= 0 else t * np.float64(10 ** -D)
        plane = np.full(ni * nj, np.nan, dtype=np.float32)
        plane[where[:n]] = y.astype(np.float32)
    plane = plane.reshape(nj, ni)
    return np.ascontiguousarray(plane[::-1]) if flip else plane


# ------------------------------------------------------------------------------------------------ fields and files of the tests
def wide_field():
    """order 0: groups of widths 0, 1, 31 and 32 behind references of 32 bits"""
    top = 2 ** 32 - 1
    f = [7] * 5 + [top - 1, top, top - 1] + [10, 10 + 2 ** 31 - 1, 11, 500] + [0, top, 12345, top - 1, 1] + [3]
    return np.array(f, dtype=np.int64), [0, 5, 8, 12, 17]


def wrap_field(g, n):
    """order 2: second differences of up to 32 bits, so that the partial sums of d and of j d pass 2^32 many times over"""
    d = g.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64)
    d[:2] = 0
    steps = np.cumsum(d) + (-3 - 5)
    steps[0] = 0
    return 5 + np.cumsum(steps)          # f[0] = 5, f[1] = -3


def malformed(kind, ni=9, nj=5, seed=4, present=None, **kw):
    """(message whose stream contradicts its header, the status bit of the condition, the words of the host's error)"""
    g = np.random.default_rng(seed)
    n = ni * nj if present is None else int(np.count_nonzero(present))
    msg = message(ni, nj, smooth_field(g, n), 2, random_bounds(g, n, 2, 9), 1.5, -2, 1, present=present, **kw)
    if kind == "lengths":
        return patched(msg, 5, lambda s: s.__setitem__(slice(42, 46), struct.pack(">I", struct.unpack_from(">I", s, 42)[0] + 1))), 1, \
            "group lengths sum to"
    if kind == "width":
        return patched(msg, 5, lambda s: s.__setitem__(35, 40)), 2, "group width of"
    assert kind == "stream"
    return patched(msg, 7, lambda s: s[:-3]), 4, "values need"


def mixed_file(south_to_north, ni=39, nj=23, seed=6, bitmaps=True):
    """the bytes of a file with a 5.0, a 5.2 and two 5.3 messages (orders 1 and 2) on one grid, their fids, and the expected planes
    (north first, as the reader returns them) from the integers that went in"""
    g = np.random.default_rng(seed)
    n = ni * nj
    fid = lambda c, p: {"discipline": 0, "parameterCategory": c, "parameterNumber": p}   # noqa: E731
    present = (g.random(n) < 0.7) if bitmaps else None
    X = g.integers(0, 2 ** 12, size=n, dtype=np.uint64)
    out = [simple_message(ni, nj, X, 12, 1.5, -2, 1, south_to_north=south_to_north, category=0, number=0)]
    fids, planes = [fid(0, 0)], [expected_plane(X.astype(np.int64), ni, nj, 1.5, -2, 1, flip=south_to_north)]
    for i, (order, masked) in enumerate(((0, False), (1, True), (2, False))):
        p = present if masked else None
        f = smooth_field(g, n if p is None else int(p.sum()), offset=5000 if order == 0 else -100 * i)
        out.append(message(ni, nj, f, order, random_bounds(g, f.size), 250.0, -1, 1, present=p, south_to_north=south_to_north,
                              category=2, number=i))
        fids.append(fid(2, i))
        planes.append(expected_plane(f, ni, nj, 250.0, -1, 1, present=p, flip=south_to_north))
    return b"".join(out), fids, planes



# ------------------------------------------------------------------------------------------------ the restatement
def _take(data, bit, n):
    """the n-bit big-endian integer at bit `bit` of the bytes `data` (bits past the end read as 0)"""
    v = 0
    for i in range(bit, bit + n):
        byte = data[i >> 3] if (i >> 3) < len(data) else 0
        v = (v << 1) | ((byte >> (7 - (i & 7))) & 1)
    return v


def _signed64(v):
    v &= MASK64
    return v - (1 << 64) if v >> 63 else v


def restate(msg):
    """A sequential decode of one 5.2 / 5.3 message in plain loops -> (f as a list of signed Python integers, (nj, ni) float32 plane in
    stream order, NaN at absent points).  Asserts where the stream contradicts the header."""
    s = ref.walk(msg)[0]
    s3, s5, s6, data = s[3], s[5], s[6], s[7][5:]
    ni, nj = struct.unpack_from(">II", s3, 30)
    count, template = struct.unpack_from(">IH", s5, 5)
    assert template in (2, 3)
    R = struct.unpack_from(">f", s5, 11)[0]
    E, D = ref.unsm(s5[15:17]), ref.unsm(s5[17:19])
    ref_bits = s5[19]
    ng, w_ref, w_bits, l_ref, l_inc, l_last, l_bits = struct.unpack_from(">IBBIBIB", s5, 31)
    order, nbytes = (s5[47], s5[48]) if template == 3 else (0, 0)
    at = 0
    extra = []
    for _ in range(order + 1 if order else 0):
        extra.append(ref.unsm(data[at:at + nbytes]) if nbytes else 0)
        at += nbytes
    bit = 8 * at
    tables = []
    for width in (ref_bits, w_bits, l_bits):
        tables.append([_take(data, bit + g * width, width) for g in range(ng)])
        bit += (ng * width + 7) // 8 * 8
    refs, ws, ls = tables
    X = []
    for g in range(ng):
        width = w_ref + ws[g]
        length = l_last if g == ng - 1 else l_ref + l_inc * ls[g]
        assert width <= 32
        for _ in range(length):
            X.append(refs[g] + _take(data, bit, width))
            bit += width
    assert len(X) == count and bit <= 8 * len(data)
    if order == 0:
        f = X
    else:
        gmin = extra[-1]
        f = []
        for k in range(count):
            if k == 0:
                f.append(extra[0])
            elif k == 1 and order == 2:
                f.append(extra[1])
            elif order == 1:
                f.append(_signed64(f[k - 1] + X[k] + gmin))
            else:
                f.append(_signed64(X[k] + gmin + 2 * f[k - 1] - f[k - 2]))
    points = ni * nj
    if s6[5] == 255:
        present = [True] * points
    else:
        present = [bool((s6[6 + (p >> 3)] >> (7 - (p & 7))) & 1) for p in range(points)]
    plane = np.full(points, np.nan, dtype=np.float32)
    k = 0
    for p in range(points):
        if present[p]:
            if k < count:
                t = np.float64(R) + np.ldexp(np.float64(f[k]), E)
                with np.errstate(all="ignore"):
                    plane[p] = np.float32(t / np.float64(10 ** D) if D >= 0 else t * np.float64(10 ** -D))
            k += 1
    return f, plane.reshape(nj, ni)


# ------------------------------------------------------------------------------------------------ a batch for the device
def layout(fields, flips=None, gap=0, lead=0, tail=0):
    """The complex-packed fields (``grib2.ComplexField``) of a call in one byte buffer and their GRIB_CFIELD table.

    Streams and bitmaps lie at 4-byte aligned offsets after ``lead`` bytes of 0xEE, with ``tail`` such bytes at the end; the planes
    lie after GUARD floats, each at a multiple of 4 floats, ``gap`` floats (a multiple of 4) between two.  tile0 and chunk0 are left
    to ``ops.grib_unpack_complex``.  -> (bytes uint8 array, table, number of floats of the whole output buffer, guards included)."""
    from py4cast_amd import ops

    assert gap % 4 == 0 and lead % 4 == 0
    flips = [False] * len(fields) if flips is None else list(flips)
    table = np.zeros(len(fields), dtype=ops.GRIB_CFIELD)
    chunks, at, dst = [b"\xee" * lead], lead, GUARD
    for i, (f, flip) in enumerate(zip(fields, flips)):
        s_off, b_off = at, -1
        chunks.append(bytes(f.stream) + b"\xee" * (-len(f.stream) % 4))
        at += len(chunks[-1])
        if f.bitmap is not None:
            b_off = at
            chunks.append(bytes(f.bitmap) + b"\xee" * (-len(f.bitmap) % 4))
            at += len(chunks[-1])
        rec = table[i]
        rec["stream_off"], rec["stream_len"], rec["bitmap_off"], rec["dst_off"] = s_off, len(f.stream), b_off, dst
        for name in ("ni", "nj", "count", "ng", "ref_bits", "w_ref", "w_bits", "l_ref", "l_inc", "l_last", "l_bits", "order", "nbytes", "ival1",
                     "ival2", "gmin", "E", "D", "R"):
            rec[name] = getattr(f, name)
        rec["flip_rows"] = int(flip)
        dst += (f.ni * f.nj + 3) // 4 * 4 + gap
    chunks.append(b"\xee" * (tail + 4))
    return np.frombuffer(b"".join(chunks), dtype=np.uint8).copy(), table, dst - gap + GUARD
