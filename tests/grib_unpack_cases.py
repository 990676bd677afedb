"""
What the tests of the GRIB reader need beyond tests/grib2_reference.py (test infrastructure, never product code; not collected):
messages around a GIVEN stream of integers -- any width from 0 to 32 bits, any R, E, D, any bitmap -- built with that module's section
builders, the expected planes, and the layout of a batch of packed fields in one byte buffer for ``ops.grib_unpack``.

The expected values everywhere are ``grib2.decode(message)[0].filled(nan).astype(float32)``: the contract of csrc/grib_unpack.hip is
that very sequence of single rounded float64 operations, so the comparison is bit for bit (``same_bits``), NaNs by position.
"""
import datetime as dt
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib2_reference as ref  # noqa: E402

SENTINEL = np.float32(-12345.678)      # what guards and gaps hold: finite, and no value any case decodes to
GUARD = 64                             # floats either side of the planes (a multiple of 4)


def stream_of(X, nbits):
    """the integers X in nbits bits each, most significant bit first, the last octet zero-padded"""
    X = np.asarray(X, dtype=np.uint64)
    if nbits == 0 or X.size == 0:
        return b""
    bits = ((X[:, None] >> np.arange(nbits - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits.reshape(-1)).tobytes()


def message(ni, nj, X, nbits, R, E, D, present=None, south_to_north=False, count=None, category=0, number=0):
    """A whole message on an nj x ni grid around the integers X (one per PRESENT point, stream order).  present: None (no bitmap,
    bitmap indicator 255) or ni*nj booleans in stream order.  count: what section 5 says (default: len(X))."""
    X = np.asarray(X, dtype=np.uint64)
    points = ni * nj
    assert X.size == (points if present is None else int(np.count_nonzero(present)))
    assert nbits == 0 or int(X.max(initial=0)) < 2 ** nbits
    stream = stream_of(X, nbits)
    if present is None:
        s6 = struct.pack(">IBB", 6, 6, 255)
    else:
        bitmap = np.packbits(np.asarray(present, dtype=np.uint8).reshape(-1)).tobytes()
        s6 = struct.pack(">IBB", 6 + len(bitmap), 6, 0) + bitmap
    when = dt.datetime(2020, 1, 1, 0)
    parts = [ref.section1(when), ref.section3(south_to_north, ni=ni, nj=nj), ref.section4(category, number, 103, (0, 2)),
             ref.section5(X.size if count is None else count, R, E, D, nbits), s6, struct.pack(">IB", 5 + len(stream), 7) + stream, b"7777"]
    return b"GRIB\x00\x00" + bytes([0, 2]) + struct.pack(">Q", 16 + sum(len(p) for p in parts)) + b"".join(parts)


def random_message(g, ni, nj, nbits, R, E, D, present=None, south_to_north=False, **kw):
    """``message`` around uniformly random nbits-bit integers, the extremes 0 and 2^nbits - 1 among them"""
    n = ni * nj if present is None else int(np.count_nonzero(present))
    X = g.integers(0, 2 ** nbits, size=n, dtype=np.uint64) if nbits else np.zeros(n, dtype=np.uint64)
    if n >= 2 and nbits:
        X[0], X[-1] = 2 ** nbits - 1, 0
    return message(ni, nj, X, nbits, R, E, D, present=present, south_to_north=south_to_north, **kw)


def expected_plane(msg, flip=False):
    """(nj, ni) float32: ``grib2.decode`` of the message, absent points NaN, rounded to float32; flipped rows with ``flip``"""
    from py4cast_amd import grib2

    with np.errstate(all="ignore"):
        plane = grib2.decode(msg)[0].filled(np.nan).astype(np.float32)
    return np.ascontiguousarray(plane[::-1]) if flip else plane


def same_bits(got, want):
    """bit for bit where ``want`` is a number, NaN exactly where it is NaN"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]))


def window_present(ni, nj, r0, r1, c0, c1):
    """a writer-style bitmap: the points of rows r0 .. r1, columns c0 .. c1 are present"""
    present = np.zeros((nj, ni), dtype=bool)
    present[r0:r1 + 1, c0:c1 + 1] = True
    return present.reshape(-1)


def layout(fields, flips=None, gap=0, lead=0, tail=0):
    """The packed fields of a call in one byte buffer and their GRIB_FIELD table.

    Streams and bitmaps lie at 4-byte aligned offsets after ``lead`` bytes of 0xEE, with ``tail`` such bytes at the end; the planes
    lie after GUARD floats, each at a multiple of 4 floats, ``gap`` floats (a multiple of 4) between two.  -> (bytes uint8 array,
    table, number of floats of the whole output buffer, guards included)."""
    from py4cast_amd import ops

    assert gap % 4 == 0 and lead % 4 == 0
    flips = [False] * len(fields) if flips is None else list(flips)
    table = np.zeros(len(fields), dtype=ops.GRIB_FIELD)
    chunks, at, dst = [b"\xee" * lead], lead, GUARD
    for i, (f, flip) in enumerate(zip(fields, flips)):
        s_off, b_off = at, -1
        chunks.append(bytes(f.stream) + b"\xee" * (-len(f.stream) % 4))
        at += len(chunks[-1])
        if f.bitmap is not None:
            b_off = at
            chunks.append(bytes(f.bitmap) + b"\xee" * (-len(f.bitmap) % 4))
            at += len(chunks[-1])
        table[i] = (s_off, len(f.stream), b_off, dst, f.ni, f.nj, f.count, f.nbits, f.E, f.D, f.R, int(flip), 0, 0)
        dst += (f.ni * f.nj + 3) // 4 * 4 + gap
    chunks.append(b"\xee" * (tail + 4))
    return np.frombuffer(b"".join(chunks), dtype=np.uint8).copy(), table, dst - gap + GUARD


def expected_buffer(table, planes, floats):
    """the whole output buffer: SENTINEL in guards, gaps and padding, every plane at its dst_off"""
    want = np.full(floats, SENTINEL, dtype=np.float32)
    for rec, plane in zip(table, planes):
        want[rec["dst_off"]:rec["dst_off"] + plane.size] = plane.reshape(-1)
    return want
