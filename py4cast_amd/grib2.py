"""
GRIB edition 2 on a regular latitude / longitude grid, as far as the forecast writer needs it (``outputs.ForecastGribWriter``):
read a template file, find the message a feature is written with, and emit a new message around a simple-packed bit stream that
``ops.grib_pack`` (csrc/grib_pack.hip) -- or ``pack_fields`` below, on the CPU -- produced.  numpy only: no eccodes, no epygram.

The layout is the WMO one (Manual on Codes I.2, FM 92).  Octets are 1-based, integers big-endian, negative values sign-and-magnitude
(the top bit of the field set): E, D, latitudes, longitudes, scale factors and scaled values.

  section 0 (16)   "GRIB"; 7 discipline; 8 edition = 2; 9-16 total length
  section 1        6-7 centre; 8-9 sub-centre; 10-11 table versions; 12 significance of the reference time; 13-14 year; 15 month;
                   16 day; 17 hour; 18 minute; 19 second; 20 production status; 21 type of data
  section 2        local use, optional: carried through untouched
  section 3 (72)   grid definition template 3.0 only: 7-10 number of points; 11-12 must be 0; 13-14 template number; 31-34 Ni;
                   35-38 Nj; 39-42 basic angle; 43-46 subdivisions; 47-50 La1; 51-54 Lo1; 56-59 La2; 60-63 Lo2; 64-67 Di; 68-71 Dj;
                   72 scanning mode.  Angles in 1e-6 degree when basic angle and subdivisions are 0 or missing.
  section 4        6-7 number of coordinate values (must be 0); 8-9 template number: 4.0 (34 octets) or 4.8 (58): 10 category;
                   11 number; 18 unit of time range; 19-22 forecast time; 23 first surface type; 24 scale factor; 25-28 scaled value;
                   29 second surface type; 4.8: 35-41 END of the interval; 42 number of time ranges (must be 1); 47 statistical
                   process; 49 unit; 50-53 length of the time range
  section 5 (21)   template 5.0: 6-9 number of packed values; 12-15 R (binary32); 16-17 E; 18-19 D; 20 nbits; 21 = 0
  section 6        6 bitmap indicator: 0 = a bitmap follows (most significant bit first, 1 = value present), 255 = none
  section 7        6.. the packed values;   section 8  "7777"

A decoded value is ``Y = (R + X 2^E) / 10^D``.

What ``Template.find`` compares, with the key names of the reference's ``feature2fid`` (io/outputs.py:325-433): ``discipline``,
``parameterCategory``, ``parameterNumber``, ``typeOfFirstFixedSurface``, ``level`` (the first surface's scaled value with its scale
factor applied; 0 where either is missing), ``typeOfSecondFixedSurface``, ``productDefinitionTemplateNumber`` and, for template 8,
``lengthOfTimeRange`` and ``typeOfStatisticalProcessing``.  ``editionNumber`` (always 2 here), ``name``, ``shortName`` (eccodes'
tables, not in the message) and ``tablesVersion`` are IGNORED.

Refused, each with the octet in the message: a grid template other than 3.0; scanning-mode bits 0x80 (points run in the -i
direction), 0x20 (adjacent points consecutive in j) and 0x10 (alternate rows reversed); a list of numbers of points; coordinate values
in section 4; a product template other than 4.0 / 4.8; more than one time range; a data representation template other than 5.0,
5.2, 5.3, 5.40, 5.41 as the source of D and nbits (these share octets 18-19 and 20); anything but 5.0, 5.2 and 5.3 on decoding; a
message with repeated sections.  Scanning-mode bit 0x40 (rows run south to north) is honoured.

Reading (``diskio.GribPlaneReader``): ``GribFile`` indexes a file, ``field_of`` hands out a message's packed stream and bitmap as
they lie in it, ``ops.grib_unpack`` (csrc/grib_unpack.hip) decodes a batch of them on the device and ``unpack_fields`` in numpy.
Complex packing (5.2) and complex packing with spatial differencing (5.3), as g2clib's ``comunpack`` reads them, go the same way:
``complex_field_of`` -> ``ComplexField``, ``ops.grib_unpack_complex`` (csrc/grib_complex.hip), ``unpack_fields``:

  section 5 (47)   template 5.2: 6-9 number of values; 12-15 R; 16-17 E; 18-19 D; 20 bits of a group reference; 21 type of original
                   values (ignored); 22 group splitting method (1 = general); 23 missing value management (0 = none); 24-31 missing
                   value substitutes (unused); 32-35 NG, number of groups; 36 reference of the group widths; 37 bits of a group width;
                   38-41 reference of the group lengths; 42 length increment; 43-46 true length of the last group; 47 bits of a
                   scaled group length
  section 5 (49)   template 5.3 adds: 48 order of the spatial differencing (1 or 2); 49 octets of each extra descriptor
  section 7        6.. 5.3 only: ival1, ival2 (order 2), gmin, sign and magnitude; then, each zero-padded to an octet: NG group
                   references, NG widths, NG scaled lengths, the values in group order (group g: len[g] integers of width[g] bits)

``width[g] = w_ref + w[g]``, ``len[g] = l_ref + l_inc * l[g]``, the last group's length is octets 43-46 whatever its stored length
says, a table of 0 bits is absent (all 0).  ``X[k] = ref[g] + value``; 5.2: f = X; 5.3 order 1: f[0] = ival1, f[k] = f[k-1] + X[k] +
gmin; order 2: f[0] = ival1, f[1] = ival2, f[k] = X[k] + gmin + 2 f[k-1] - f[k-2]; integer arithmetic modulo 2^64, f signed;
``Y = (R + f 2^E) / 10^D``.  The writer's opt-in complex packing (``pack_complex``, ``encode(..., order=, ref_bits=)``,
``ops.grib_pack_complex``, csrc/grib_pack_complex.hip) writes these templates with groups of 32 values: l_ref = 32, l_inc = 1, a
table of lengths of 0 bits, w_ref = 0, widths in 6 bits, descriptors of 4 octets; ``packing_of`` tells which packing a template
message asks for.  Still out of scope and refused: 5.40, 5.41, 5.42, missing value management 1 and 2, group splitting
other than the general one.  Messages are found by the numeric keys above, never by ``shortName``.
"""
import datetime as dt
import math
import struct
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

IGNORED_KEYS = ("editionNumber", "name", "shortName", "tablesVersion")
MATCHED_KEYS = ("discipline", "parameterCategory", "parameterNumber", "typeOfFirstFixedSurface", "level", "typeOfSecondFixedSurface",
                "productDefinitionTemplateNumber", "lengthOfTimeRange", "typeOfStatisticalProcessing")
D_NBITS_TEMPLATES = (0, 2, 3, 40, 41)
UNIT_MINUTE, UNIT_HOUR = 0, 1
MAX_D = 15
COMPLEX_TEMPLATES = (2, 3)


class GribError(ValueError):
    pass


# ------------------------------------------------------------------------------------------------ octets
def _u(b: bytes, octet: int, n: int) -> int:
    return int.from_bytes(b[octet - 1:octet - 1 + n], "big")


def _s(b: bytes, octet: int, n: int) -> int:
    raw = _u(b, octet, n)
    top = 1 << (8 * n - 1)
    return -(raw & (top - 1)) if raw & top else raw


def _missing(b: bytes, octet: int, n: int) -> bool:
    return _u(b, octet, n) == (1 << (8 * n)) - 1


def _put_u(b: bytearray, octet: int, n: int, value: int) -> None:
    if not 0 <= value < 1 << (8 * n):
        raise GribError(f"{value} does not fit the {n} octets at {octet}")
    b[octet - 1:octet - 1 + n] = int(value).to_bytes(n, "big")


def _put_s(b: bytearray, octet: int, n: int, value: int) -> None:
    top = 1 << (8 * n - 1)
    if abs(value) >= top:
        raise GribError(f"{value} does not fit the {n} octets at {octet}")
    _put_u(b, octet, n, (top | -value) if value < 0 else value)


# ------------------------------------------------------------------------------------------------ messages
class Message:
    """One GRIB2 message: ``discipline``, ``sections`` (number -> the section's bytes, length prefix included; 0 and 8 too) and the
    parsed ``keys``."""

    def __init__(self, raw: bytes):
        if raw[:4] != b"GRIB" or len(raw) < 20:
            raise GribError("not a GRIB message")
        if raw[7] != 2:
            raise GribError(f"section 0 octet 8: edition {raw[7]}, only edition 2 is read")
        total = _u(raw, 9, 8)
        if total != len(raw) or raw[-4:] != b"7777":
            raise GribError(f"section 0 octets 9-16: length {total} of a message of {len(raw)} octets (or no 7777 at its end)")
        self.raw = bytes(raw)
        self.discipline = raw[6]
        self.sections: Dict[int, bytes] = {0: bytes(raw[:16]), 8: b"7777"}
        at = 16
        while at < total - 4:
            length, number = _u(raw, at + 1, 4), raw[at + 4]
            if length < 5 or at + length > total - 4 or not 1 <= number <= 7:
                raise GribError(f"section {number} of {length} octets at offset {at} does not fit the message")
            if number in self.sections:
                raise GribError(f"section {number} is repeated: messages with several fields are not read")
            self.sections[number] = bytes(raw[at:at + length])
            at += length
        for number in (1, 3, 4, 5, 6, 7):
            if number not in self.sections:
                raise GribError(f"section {number} is missing")
        self.keys = _keys(self)

    def __repr__(self):
        k = self.keys
        return (f"Message(discipline={k['discipline']}, category={k['parameterCategory']}, number={k['parameterNumber']}, "
                f"template=4.{k['productDefinitionTemplateNumber']})")


def _datetime(b: bytes, octet: int) -> Optional[dt.datetime]:
    try:
        return dt.datetime(_u(b, octet, 2), b[octet + 1], b[octet + 2], b[octet + 3], b[octet + 4], b[octet + 5])
    except ValueError:
        return None


def _keys(m: Message) -> dict:
    s1, s3, s4, s5, s6 = (m.sections[i] for i in (1, 3, 4, 5, 6))
    k = {"discipline": m.discipline, "editionNumber": 2, "centre": _u(s1, 6, 2), "subCentre": _u(s1, 8, 2), "tablesVersion": s1[9],
         "referenceTime": _datetime(s1, 13), "hasLocalSection": 2 in m.sections,
         "gridDefinitionTemplateNumber": _u(s3, 13, 2), "numberOfDataPoints": _u(s3, 7, 4),
         "numberOfCoordinateValues": _u(s4, 6, 2), "productDefinitionTemplateNumber": _u(s4, 8, 2)}
    if k["gridDefinitionTemplateNumber"] == 0 and len(s3) >= 72:
        k.update(Ni=_u(s3, 31, 4), Nj=_u(s3, 35, 4), basicAngle=_u(s3, 39, 4), subdivisions=_u(s3, 43, 4), La1=_s(s3, 47, 4),
                 Lo1=_s(s3, 51, 4), La2=_s(s3, 56, 4), Lo2=_s(s3, 60, 4), Di=_u(s3, 64, 4), Dj=_u(s3, 68, 4), scanningMode=s3[71])
    if k["productDefinitionTemplateNumber"] in (0, 8) and len(s4) >= 34:
        scale, value = _s(s4, 24, 1), _s(s4, 25, 4)
        absent = _missing(s4, 24, 1) or _missing(s4, 25, 4)
        k.update(parameterCategory=s4[9], parameterNumber=s4[10], indicatorOfUnitOfTimeRange=s4[17], forecastTime=_u(s4, 19, 4),
                 typeOfFirstFixedSurface=s4[22], typeOfSecondFixedSurface=s4[28],
                 level=0 if absent else value / 10 ** scale)
        if k["productDefinitionTemplateNumber"] == 8 and len(s4) >= 58:
            k.update(endOfInterval=_datetime(s4, 35), numberOfTimeRanges=s4[41], typeOfStatisticalProcessing=s4[46],
                     indicatorOfUnitForTimeRange=s4[48], lengthOfTimeRange=_u(s4, 50, 4))
    k.update(numberOfValues=_u(s5, 6, 4), dataRepresentationTemplateNumber=_u(s5, 10, 2), bitMapIndicator=s6[5])
    if k["dataRepresentationTemplateNumber"] in D_NBITS_TEMPLATES and len(s5) >= 20:
        k.update(referenceValue=struct.unpack(">f", s5[11:15])[0], binaryScaleFactor=_s(s5, 16, 2), decimalScaleFactor=_s(s5, 18, 2),
                 bitsPerValue=s5[19])
    return k


def parse_messages(data: bytes) -> List[Message]:
    out, at = [], 0
    while True:
        at = data.find(b"GRIB", at)
        if at < 0 or at + 16 > len(data):
            return out
        total = _u(data[at:at + 16], 9, 8)
        out.append(Message(data[at:at + total]))
        at += total


def read_messages(path) -> List[Message]:
    """Walk a GRIB2 file into its messages."""
    with open(path, "rb") as f:
        return parse_messages(f.read())


def check_grid(m: Message) -> None:
    """Raise for a grid this module does not write on (module docstring)."""
    s3 = m.sections[3]
    number = _u(s3, 13, 2)
    if number != 0 or len(s3) < 72:
        raise GribError(f"section 3 octets 13-14: grid definition template 3.{number}; only 3.0 (regular latitude / longitude) is written")
    if s3[10] != 0 or s3[11] != 0:
        raise GribError(f"section 3 octets 11-12: a list of numbers of points ({s3[10]}, {s3[11]}) is not read")
    mode = s3[71]
    for bit, what in ((0x80, "points are scanned in the -i direction"), (0x20, "adjacent points are consecutive in j"),
                      (0x10, "alternate rows are scanned in the opposite direction")):
        if mode & bit:
            raise GribError(f"section 3 octet 72: scanning mode 0x{mode:02x}: bit 0x{bit:02x} ({what}) is not written")
    if m.keys["Ni"] * m.keys["Nj"] != m.keys["numberOfDataPoints"]:
        raise GribError(f"section 3 octets 7-10: {m.keys['numberOfDataPoints']} points on a grid of {m.keys['Ni']} x {m.keys['Nj']}")


def check_product(m: Message) -> None:
    s4 = m.sections[4]
    if _u(s4, 6, 2) != 0:
        raise GribError(f"section 4 octets 6-7: {_u(s4, 6, 2)} coordinate values; vertical coordinate lists are not written")
    number = _u(s4, 8, 2)
    if number not in (0, 8) or len(s4) < (34 if number == 0 else 58):
        raise GribError(f"section 4 octets 8-9: product definition template 4.{number}; only 4.0 and 4.8 are written")
    if number == 8 and s4[41] != 1:
        raise GribError(f"section 4 octet 42: {s4[41]} time ranges; exactly one is written")


def spec_of(m: Message) -> Tuple[int, int]:
    """(D, nbits) of a template message: octets 18-19 and 20 of section 5, where templates 5.0, 5.2, 5.3, 5.40 and 5.41 keep them"""
    s5 = m.sections[5]
    number = _u(s5, 10, 2)
    if number not in D_NBITS_TEMPLATES or len(s5) < 20:
        raise GribError(f"section 5 octets 10-11: data representation template 5.{number}: D and nbits are taken from 5.0, 5.2, 5.3, 5.40, 5.41")
    D, nbits = _s(s5, 18, 2), s5[19]
    if abs(D) > MAX_D or not 1 <= nbits <= 32:
        raise GribError(f"section 5 octets 18-20: D = {D}, nbits = {nbits}: |D| <= {MAX_D} and 1 <= nbits <= 32 are packed")
    return D, nbits


def grid_of(m: Message):
    """(Ni, Nj, lat, lon, scanning mode): ``lat[r]`` the latitude of stream row r, ``lon[c]`` the longitude of stream column c, degrees;
    longitudes are wrapped into [-180, 180)"""
    check_grid(m)
    k = m.keys
    basic, sub = k["basicAngle"], k["subdivisions"]
    unit = 1e-6 if basic in (0, 0xFFFFFFFF) or sub in (0, 0xFFFFFFFF) else basic / sub
    lat = np.linspace(k["La1"] * unit, k["La2"] * unit, k["Nj"])
    lo1, lo2 = k["Lo1"] * unit, k["Lo2"] * unit
    if lo2 < lo1:
        lo2 += 360.0
    lon = (np.linspace(lo1, lo2, k["Ni"]) + 180.0) % 360.0 - 180.0
    south_to_north = bool(k["scanningMode"] & 0x40)
    if k["Nj"] > 1 and (lat[-1] > lat[0]) != south_to_north:
        raise GribError(f"section 3 octet 72: scanning mode 0x{k['scanningMode']:02x} against La1 = {lat[0]}, La2 = {lat[-1]}")
    return k["Ni"], k["Nj"], lat, lon, k["scanningMode"]


def find_message(messages: Sequence[Message], fid: dict, where) -> Message:
    """The first of ``messages`` whose keys equal those of ``fid``: MATCHED_KEYS are compared, IGNORED_KEYS are not, any other key is
    refused.  ``where`` names the file in the KeyError."""
    unknown = sorted(set(fid) - set(MATCHED_KEYS) - set(IGNORED_KEYS))
    if unknown:
        raise GribError(f"keys {unknown} are not matched")
    wanted = {k: v for k, v in fid.items() if k in MATCHED_KEYS}
    for m in messages:
        if all(k in m.keys and m.keys[k] == v for k, v in wanted.items()):
            return m
    raise KeyError(f"{where}: no message with {wanted}")


class Template:
    """The messages of a template GRIB2 file; every one of them must be on a grid this module writes on."""

    def __init__(self, path):
        self.path = path
        self.messages = read_messages(path)
        if not self.messages:
            raise GribError(f"{path}: no GRIB2 message")
        for m in self.messages:
            check_grid(m)

    def find(self, fid: dict) -> Message:
        """The first message whose keys equal those of ``fid`` (module docstring: which are compared, which ignored)."""
        return find_message(self.messages, fid, self.path)

    def grid(self, message: Optional[Message] = None):
        return grid_of(self.messages[0] if message is None else message)


def match_latlon(grid_lat, grid_lon, lat: np.ndarray, lon: np.ndarray, what="dataset") -> Tuple[int, int, int, int]:
    """io/outputs.py:269-322: where the forecast grid (``grid_lat``, ``grid_lon``: any shape) sits in the template's vectors, compared
    after rounding to 5 decimals -> (first row, last row, first column, last column) of the template grid, in its stream order.  The
    forecast grid must lie inside the template's or equal it."""
    grid_lat, grid_lon = np.asarray(grid_lat, dtype=np.float64), np.asarray(grid_lon, dtype=np.float64)
    error = ValueError(f"Lat/Lon dims of the {what} do not fit in template grid, cannot write grib.")
    if not (lat.min() <= grid_lat.min() and lat.max() >= grid_lat.max() and lon.min() <= grid_lon.min() and lon.max() >= grid_lon.max()):
        raise error
    found = [np.where(np.round(vec, 5) == round(float(v), 5))[0]
             for vec, v in ((lat, grid_lat.min()), (lat, grid_lat.max()), (lon, grid_lon.min()), (lon, grid_lon.max()))]
    if any(len(f) != 1 for f in found):
        raise error
    a, b, c, d = (int(f[0]) for f in found)
    return min(a, b), max(a, b), min(c, d), max(c, d)


@lru_cache(maxsize=16)
def _bitmap(Nj: int, Ni: int, window: Tuple[int, int, int, int]) -> Optional[bytes]:
    r0, r1, c0, c1 = window
    if (r0, r1, c0, c1) == (0, Nj - 1, 0, Ni - 1):
        return None
    present = np.zeros((Nj, Ni), dtype=np.uint8)
    present[r0:r1 + 1, c0:c1 + 1] = 1
    return np.packbits(present.reshape(-1)).tobytes()


def _time_in_unit(delta: dt.timedelta, what: str) -> Tuple[int, int]:
    seconds = delta.total_seconds()
    if seconds < 0 or seconds != int(seconds) or int(seconds) % 60:
        raise GribError(f"{what} {delta}: whole minutes, not negative, are written")
    seconds = int(seconds)
    return (UNIT_HOUR, seconds // 3600) if seconds % 3600 == 0 else (UNIT_MINUTE, seconds // 60)


COMPLEX_GROUP = 32        # values of a group of the complex packing written here
COMPLEX_W_BITS = 6        # bits of a stored group width
COMPLEX_PARAMS = 11       # int32 words of a params record of ``ops.grib_pack_complex``


def check_complex(nbits: int, order: int) -> None:
    """The limits of the complex packing written here: order 0 (5.2) takes 1 .. 32 bits, orders 1 and 2 (5.3) need nbits + order <= 31,
    so that every descriptor fits sign and magnitude in 4 octets and every X', reference and width fits 32 bits"""
    if order not in (0, 1, 2):
        raise GribError(f"spatial differencing of order {order}: 0 (template 5.2), 1 and 2 (template 5.3) are written")
    if not 1 <= nbits <= 32 or (order and nbits + order > 31):
        raise GribError(f"nbits = {nbits} at order {order}: 1 <= nbits <= 32 at order 0, nbits + order <= 31 at orders 1 and 2")


def complex_capacity(N: int, nbits: int, order: int) -> int:
    """the worst case of one field's payload, rounded up to 4 (p4c_grib_pack_complex_capacity sums these over a call's fields)"""
    ng = (N + COMPLEX_GROUP - 1) // COMPLEX_GROUP
    octets = (4 * (order + 1) if order else 0) + 4 * ng + (COMPLEX_W_BITS * ng + 7) // 8 + 4 * ng * (nbits + order)
    return (octets + 3) // 4 * 4


def packing_of(m: Message) -> Optional[int]:
    """How a template message is packed, for the writer's ``packing="template"``: None for simple packing (5.0), the order of the
    spatial differencing for complex packing: 0 for 5.2, octet 48 (1 or 2) for 5.3.  Anything else raises with its octet."""
    s5 = m.sections[5]
    number = _u(s5, 10, 2) if len(s5) >= 11 else -1
    if number == 0:
        return None
    if number not in COMPLEX_TEMPLATES:
        raise GribError(f"section 5 octets 10-11: data representation template 5.{number}; a template message in 5.0, 5.2 or 5.3 is followed")
    octets = 47 if number == 2 else 49
    if len(s5) < octets:
        raise GribError(f"section 5 octets 1-4: {len(s5)} octets; template 5.{number} has {octets}")
    if number == 2:
        return 0
    if s5[47] not in (1, 2):
        raise GribError(f"section 5 octet 48: spatial differencing of order {s5[47]}; 1 and 2 are written")
    return int(s5[47])


def complex_section5(count: int, R: float, E: int, D: int, order: int, ref_bits: int) -> bytearray:
    """Section 5 of a field as ``pack_complex`` lays it out: template 5.2 (order 0, 47 octets) or 5.3 (49 octets); general group
    splitting, no missing value management, groups of 32 values with no table of lengths (l_ref = 32, l_inc = 1, l_bits = 0), widths in
    6 bits from 0, descriptors of 4 octets"""
    ng = (count + COMPLEX_GROUP - 1) // COMPLEX_GROUP
    s5 = bytearray(49 if order else 47)
    _put_u(s5, 1, 4, len(s5))
    s5[4] = 5
    _put_u(s5, 6, 4, count)
    _put_u(s5, 10, 2, 3 if order else 2)
    s5[11:15] = struct.pack(">f", R)
    _put_s(s5, 16, 2, E)
    _put_s(s5, 18, 2, D)
    s5[19] = ref_bits
    s5[20] = 0                         # type of original values: floating point
    s5[21] = 1                         # general group splitting
    s5[22] = 0                         # no missing value management
    _put_u(s5, 32, 4, ng)
    s5[35], s5[36] = 0, COMPLEX_W_BITS
    _put_u(s5, 38, 4, COMPLEX_GROUP)
    s5[41] = 1
    _put_u(s5, 43, 4, count - COMPLEX_GROUP * (ng - 1) if ng else 0)
    s5[46] = 0
    if order:
        s5[47], s5[48] = order, 4
    return s5


def encode(template_message: Message, basis: dt.datetime, term: dt.timedelta, *, cumulative: Optional[dt.timedelta] = None,
           window: Tuple[int, int, int, int], packed: bytes, R: float, E: int, D: int, nbits: int, order: Optional[int] = None,
           ref_bits: int = 0) -> bytes:
    """A new message: sections 0-4 of ``template_message`` with the reference time (``basis``) and the forecast time (``term``; for
    template 4.8 the interval of length ``cumulative`` that ENDS at basis + term) patched in, and new sections 5-7 around ``packed``,
    the simple-packed stream of the ``window`` (first row, last row, first column, last column of the template grid in stream order;
    the points outside it are absent in the bitmap).  With ``order`` (0: template 5.2; 1, 2: template 5.3) ``packed`` is the payload
    of ``pack_complex`` / ``ops.grib_pack_complex`` and ``ref_bits`` its octet 20: section 5 then has 47 or 49 octets and says groups
    of 32 values (``complex_section5``)."""
    m = template_message
    check_grid(m)
    check_product(m)
    Ni, Nj = m.keys["Ni"], m.keys["Nj"]
    r0, r1, c0, c1 = window
    if not (0 <= r0 <= r1 < Nj and 0 <= c0 <= c1 < Ni):
        raise GribError(f"window {window} on a grid of {Nj} x {Ni}")
    if abs(D) > MAX_D or not 1 <= nbits <= 32:
        raise GribError(f"D = {D}, nbits = {nbits}: |D| <= {MAX_D} and 1 <= nbits <= 32 are packed")
    count = (r1 - r0 + 1) * (c1 - c0 + 1)
    packed = bytes(packed)
    if order is not None:
        check_complex(nbits, order)
        ng = (count + COMPLEX_GROUP - 1) // COMPLEX_GROUP
        head = (4 * (order + 1) if order else 0) + (ng * ref_bits + 7) // 8 + (ng * COMPLEX_W_BITS + 7) // 8
        if not 0 <= ref_bits <= 32 or not head <= len(packed) <= complex_capacity(count, nbits, order):
            raise GribError(f"{len(packed)} octets of payload, {ref_bits} bits per group reference for {count} values of {nbits} bits "
                            f"at order {order}")
    elif len(packed) != (count * nbits + 7) // 8:
        raise GribError(f"{len(packed)} packed octets for {count} values of {nbits} bits")
    s1 = bytearray(m.sections[1])
    _put_u(s1, 13, 2, basis.year)
    for i, v in enumerate((basis.month, basis.day, basis.hour, basis.minute, basis.second)):
        s1[14 + i] = v
    s4 = bytearray(m.sections[4])
    if m.keys["productDefinitionTemplateNumber"] == 8:
        if cumulative is None:
            raise GribError("template 4.8 needs the cumulative duration")
        unit, value = _time_in_unit(term - cumulative, "start of the interval")
        end = basis + term
        _put_u(s4, 35, 2, end.year)
        for i, v in enumerate((end.month, end.day, end.hour, end.minute, end.second)):
            s4[36 + i] = v
        lunit, length = _time_in_unit(cumulative, "cumulative duration")
        s4[48] = lunit
        _put_u(s4, 50, 4, length)
    else:
        unit, value = _time_in_unit(term, "term")
    s4[17] = unit
    _put_u(s4, 19, 4, value)
    if order is not None:
        s5 = complex_section5(count, R, E, D, order, ref_bits)
    else:
        s5 = bytearray(21)
        _put_u(s5, 1, 4, 21)
        s5[4] = 5
        _put_u(s5, 6, 4, count)
        s5[11:15] = struct.pack(">f", R)
        _put_s(s5, 16, 2, E)
        _put_s(s5, 18, 2, D)
        s5[19] = nbits
    bitmap = _bitmap(Nj, Ni, (r0, r1, c0, c1))
    s6 = bytearray(6)
    _put_u(s6, 1, 4, 6 + (len(bitmap) if bitmap is not None else 0))
    s6[4], s6[5] = 6, (255 if bitmap is None else 0)
    s7 = bytearray(5)
    _put_u(s7, 1, 4, 5 + len(packed))
    s7[4] = 7
    body = [bytes(s1)] + ([m.sections[2]] if 2 in m.sections else []) + [m.sections[3], bytes(s4), bytes(s5), bytes(s6), bitmap or b"",
                                                                       bytes(s7), packed, b"7777"]
    s0 = bytearray(m.sections[0])
    _put_u(s0, 9, 8, 16 + sum(len(b) for b in body))
    return bytes(s0) + b"".join(body)


def unpack_bits(data: bytes, count: int, nbits: int) -> np.ndarray:
    """``count`` unsigned integers of ``nbits`` bits, most significant bit first -> uint64"""
    bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8), count=count * nbits).reshape(count, nbits).astype(np.uint64)
    return (bits << np.arange(nbits - 1, -1, -1, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def decode(message) -> Tuple[np.ma.MaskedArray, dict]:
    """A simple-packed (5.0) or complex-packed (5.2, 5.3) message on a 3.0 grid -> ((Nj, Ni) masked float64 in stream order, the
    parsed keys).  For 5.2 / 5.3 this is the float64 statement of the decode's contract (``complex_integers``)."""
    m = message if isinstance(message, Message) else Message(message)
    check_grid(m)
    k = m.keys
    if k["dataRepresentationTemplateNumber"] in COMPLEX_TEMPLATES:
        cf = complex_field_of(m)
        present = np.ones(cf.nj * cf.ni, dtype=bool) if cf.bitmap is None else \
            np.unpackbits(np.frombuffer(cf.bitmap, dtype=np.uint8), count=cf.nj * cf.ni).astype(bool)
        values = np.zeros(cf.nj * cf.ni, dtype=np.float64)
        with np.errstate(all="ignore"):
            scaled = float(cf.R) + np.ldexp(complex_integers(cf).astype(np.float64), cf.E)
            values[present] = scaled / float(10 ** cf.D) if cf.D >= 0 else scaled * float(10 ** -cf.D)
        return np.ma.MaskedArray(values.reshape(cf.nj, cf.ni), mask=~present.reshape(cf.nj, cf.ni)), k
    if k["dataRepresentationTemplateNumber"] != 0:
        raise GribError(f"section 5 octets 10-11: data representation template 5.{k['dataRepresentationTemplateNumber']}; only 5.0, 5.2 "
                        f"and 5.3 are decoded")
    Ni, Nj, count, nbits = k["Ni"], k["Nj"], k["numberOfValues"], k["bitsPerValue"]
    if k["bitMapIndicator"] == 255:
        present = np.ones(Nj * Ni, dtype=bool)
    elif k["bitMapIndicator"] == 0:
        present = np.unpackbits(np.frombuffer(m.sections[6][6:], dtype=np.uint8), count=Nj * Ni).astype(bool)
    else:
        raise GribError(f"section 6 octet 6: bitmap indicator {k['bitMapIndicator']}")
    if int(present.sum()) != count:
        raise GribError(f"section 5 octets 6-9: {count} values for {int(present.sum())} points present")
    X = unpack_bits(m.sections[7][5:], count, nbits).astype(np.float64) if nbits else np.zeros(count)
    values = np.zeros(Nj * Ni, dtype=np.float64)
    D = k["decimalScaleFactor"]
    scaled = float(k["referenceValue"]) + np.ldexp(X, k["binaryScaleFactor"])
    values[present] = scaled / float(10 ** D) if D >= 0 else scaled * float(10 ** -D)
    return np.ma.MaskedArray(values.reshape(Nj, Ni), mask=~present.reshape(Nj, Ni)), k


# ------------------------------------------------------------------------------------------------ reading: the host side
# Reading keeps the numeric work off the host: ``field_of`` hands out the packed stream and the bitmap of a message as they lie in
# the file, ``ops.grib_unpack`` (csrc/grib_unpack.hip) decodes a whole batch of them on the device, ``unpack_fields`` does the
# same in numpy.  Messages are found by the numeric MATCHED_KEYS only: ``shortName``, which the reference selects by, comes from
# eccodes' tables and is not in a message (``outputs.grib_fid`` gives the numeric keys of the Titan features).
@dataclass(frozen=True)
class PackedField:
    """What the decoder needs of one simple-packed message; ``stream`` (section 7 from octet 6) and ``bitmap`` (section 6 from
    octet 7, None without one) are memoryviews into the message's sections, not copies."""
    stream: memoryview
    bitmap: Optional[memoryview]
    ni: int
    nj: int
    count: int
    nbits: int
    R: float
    E: int
    D: int
    scanning_mode: int

    @property
    def south_to_north(self) -> bool:
        return bool(self.scanning_mode & 0x40)


def field_of(message) -> PackedField:
    """The packed field of a message on a 3.0 grid.  Refused, each with its octet: everything ``check_grid`` refuses; a data
    representation template other than 5.0 (5.2, 5.3, 5.40, 5.41, 5.42 are out of scope); a bitmap indicator other than 0 or 255;
    nbits > 32; |D| > 15; a bitmap shorter than the grid or whose population differs from the number of packed values; without a
    bitmap, a number of values other than the number of points; a section 7 shorter than ceil(count * nbits / 8)."""
    m = message if isinstance(message, Message) else Message(message)
    check_grid(m)
    k = m.keys
    number = k["dataRepresentationTemplateNumber"]
    if number != 0 or len(m.sections[5]) < 20:
        raise GribError(f"section 5 octets 10-11: data representation template 5.{number}; only 5.0 (simple packing) is decoded, "
                        f"5.2, 5.3, 5.40, 5.41 and 5.42 are out of scope")
    ni, nj, count, nbits, D = k["Ni"], k["Nj"], k["numberOfValues"], k["bitsPerValue"], k["decimalScaleFactor"]
    if nbits > 32:
        raise GribError(f"section 5 octet 20: {nbits} bits per value; 0 .. 32 are decoded")
    if abs(D) > MAX_D:
        raise GribError(f"section 5 octets 18-19: D = {D}; |D| <= {MAX_D} is decoded")
    points = ni * nj
    s6, s7 = m.sections[6], m.sections[7]
    bitmap = None
    if k["bitMapIndicator"] == 0:
        need = (points + 7) // 8
        if len(s6) - 6 < need:
            raise GribError(f"section 6 octets 1-4: a bitmap of {len(s6) - 6} octets for {points} points")
        bitmap = memoryview(s6)[6:6 + need]
        present = (int.from_bytes(bitmap, "big") >> (8 * need - points)).bit_count()
        if present != count:
            raise GribError(f"section 5 octets 6-9: {count} values for {present} points present in the bitmap")
    elif k["bitMapIndicator"] == 255:
        if count != points:
            raise GribError(f"section 5 octets 6-9: {count} values for {points} points and no bitmap")
    else:
        raise GribError(f"section 6 octet 6: bitmap indicator {k['bitMapIndicator']}; 0 (a bitmap follows) and 255 (none) are read")
    if len(s7) - 5 < (count * nbits + 7) // 8:
        raise GribError(f"section 7 octets 1-4: {len(s7) - 5} octets of data for {count} values of {nbits} bits")
    return PackedField(memoryview(s7)[5:], bitmap, ni, nj, count, nbits, float(k["referenceValue"]), k["binaryScaleFactor"], D,
                       k["scanningMode"])


@dataclass(frozen=True)
class ComplexField:
    """What the decoder needs of one complex-packed message (5.2: ``order`` 0; 5.3: ``order`` 1 or 2); ``stream`` (section 7 from
    octet 6: descriptors, group tables and values) and ``bitmap`` (section 6 from octet 7, None without one) are memoryviews into
    the message's sections, not copies.  ``ival1``, ``ival2`` and ``gmin`` are parsed here, like R, E and D; 0 where the template
    has none."""
    stream: memoryview
    bitmap: Optional[memoryview]
    ni: int
    nj: int
    count: int
    R: float
    E: int
    D: int
    scanning_mode: int
    ng: int          # octets 32-35
    ref_bits: int    # octet 20
    w_ref: int       # octet 36
    w_bits: int      # octet 37
    l_ref: int       # octets 38-41
    l_inc: int       # octet 42
    l_last: int      # octets 43-46
    l_bits: int      # octet 47
    order: int       # octet 48; 0 for template 5.2
    nbytes: int      # octet 49; 0 for template 5.2
    ival1: int
    ival2: int
    gmin: int

    @property
    def south_to_north(self) -> bool:
        return bool(self.scanning_mode & 0x40)

    @property
    def template(self) -> int:
        return 3 if self.order else 2

    @property
    def descriptor_octets(self) -> int:
        return (self.order + 1) * self.nbytes if self.order else 0

    def table_bits(self) -> Tuple[int, int, int, int]:
        """the first bit of the group references, of the widths, of the scaled lengths and of the values in ``stream``"""
        ref = 8 * self.descriptor_octets
        width = ref + 8 * ((self.ng * self.ref_bits + 7) // 8)
        length = width + 8 * ((self.ng * self.w_bits + 7) // 8)
        return ref, width, length, length + 8 * ((self.ng * self.l_bits + 7) // 8)


def complex_field_of(message) -> ComplexField:
    """The packed field of a complex-packed message on a 3.0 grid.  Refused, each with its octet: everything ``check_grid`` refuses; a
    data representation template other than 5.2 / 5.3; a section 5 shorter than 47 / 49 octets; more than 32 bits for a group
    reference, width or scaled length (octets 20, 37, 47); a group splitting method other than 1 (octet 22); missing value management
    (octet 23); an order outside 1 .. 2 (octet 48); descriptors of more than 4 octets (octet 49; with 0 the three are 0); no group for
    count > 0; |D| > 15; the bitmap conditions of ``field_of``; a section 7 shorter than the descriptors and the three padded tables."""
    m = message if isinstance(message, Message) else Message(message)
    check_grid(m)
    k = m.keys
    s5, s6, s7 = m.sections[5], m.sections[6], m.sections[7]
    number = k["dataRepresentationTemplateNumber"]
    if number not in COMPLEX_TEMPLATES:
        raise GribError(f"section 5 octets 10-11: data representation template 5.{number}; 5.2 and 5.3 (complex packing) are decoded here")
    octets = 47 if number == 2 else 49
    if len(s5) < octets:
        raise GribError(f"section 5 octets 1-4: {len(s5)} octets; template 5.{number} has {octets}")
    ni, nj, count, D = k["Ni"], k["Nj"], k["numberOfValues"], k["decimalScaleFactor"]
    for octet, what in ((20, "a group reference"), (37, "a group width"), (47, "a scaled group length")):
        if s5[octet - 1] > 32:
            raise GribError(f"section 5 octet {octet}: {s5[octet - 1]} bits for {what}; 0 .. 32 are decoded")
    if s5[21] != 1:
        raise GribError(f"section 5 octet 22: group splitting method {s5[21]}; only 1 (general group splitting) is decoded")
    if s5[22] != 0:
        raise GribError(f"section 5 octet 23: missing value management {s5[22]}; primary and secondary missing values are out of scope")
    order = nbytes = 0
    if number == 3:
        order, nbytes = s5[47], s5[48]
        if not 1 <= order <= 2:
            raise GribError(f"section 5 octet 48: spatial differencing of order {order}; 1 and 2 are decoded")
        if nbytes > 4:
            raise GribError(f"section 5 octet 49: {nbytes} octets per extra descriptor; 0 .. 4 are decoded")
    ng = _u(s5, 32, 4)
    if ng == 0 and count > 0:
        raise GribError(f"section 5 octets 32-35: no group for {count} values")
    if abs(D) > MAX_D:
        raise GribError(f"section 5 octets 18-19: D = {D}; |D| <= {MAX_D} is decoded")
    points = ni * nj
    bitmap = None
    if k["bitMapIndicator"] == 0:
        need = (points + 7) // 8
        if len(s6) - 6 < need:
            raise GribError(f"section 6 octets 1-4: a bitmap of {len(s6) - 6} octets for {points} points")
        bitmap = memoryview(s6)[6:6 + need]
        present = (int.from_bytes(bitmap, "big") >> (8 * need - points)).bit_count()
        if present != count:
            raise GribError(f"section 5 octets 6-9: {count} values for {present} points present in the bitmap")
    elif k["bitMapIndicator"] == 255:
        if count != points:
            raise GribError(f"section 5 octets 6-9: {count} values for {points} points and no bitmap")
    else:
        raise GribError(f"section 6 octet 6: bitmap indicator {k['bitMapIndicator']}; 0 (a bitmap follows) and 255 (none) are read")
    stream = memoryview(s7)[5:]
    descriptors = [_s(stream, 1 + i * nbytes, nbytes) if nbytes and len(stream) >= (i + 1) * nbytes else 0 for i in range(order + 1 if order else 0)]
    ival1 = descriptors[0] if order else 0
    ival2 = descriptors[1] if order == 2 else 0
    gmin = descriptors[-1] if order else 0
    f = ComplexField(stream, bitmap, ni, nj, count, float(k["referenceValue"]), k["binaryScaleFactor"], D, k["scanningMode"], ng,
                     s5[19], s5[35], s5[36], _u(s5, 38, 4), s5[41], _u(s5, 43, 4), s5[46], order, nbytes, ival1, ival2, gmin)
    need = f.table_bits()[3] // 8
    if len(stream) < need:
        raise GribError(f"section 7 octets 1-4: {len(stream)} octets of data for {need} octets of descriptors and group tables")
    return f


def _integers_at(bits: np.ndarray, starts: np.ndarray, width: int) -> np.ndarray:
    """the ``width``-bit integers that start at the bits ``starts`` of the 0/1 array ``bits``, most significant bit first -> uint64"""
    if width == 0 or starts.size == 0:
        return np.zeros(starts.size, dtype=np.uint64)
    picked = bits[starts[:, None] + np.arange(width, dtype=np.int64)].astype(np.uint64)
    return (picked << np.arange(width - 1, -1, -1, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def complex_integers(f: ComplexField) -> np.ndarray:
    """The ``count`` integers f[k] of a complex-packed field (module docstring) -> int64; all sums modulo 2^64.  Raises GribError when
    the stream contradicts the header: the group lengths do not sum to count, a group width above 32, values past the stream's end
    (bits 1, 2, 4 of the device's status word)."""
    bits = np.unpackbits(np.frombuffer(f.stream, dtype=np.uint8))
    at_ref, at_width, at_length, at_values = f.table_bits()
    if at_values > bits.size:
        raise GribError(f"a stream of {bits.size // 8} octets is shorter than its descriptors and group tables ({at_values // 8} octets)")
    g = np.arange(f.ng, dtype=np.int64)
    ref = _integers_at(bits, at_ref + g * f.ref_bits, f.ref_bits)
    width = f.w_ref + _integers_at(bits, at_width + g * f.w_bits, f.w_bits).astype(np.int64)
    length = f.l_ref + f.l_inc * _integers_at(bits, at_length + g * f.l_bits, f.l_bits).astype(np.int64)
    if f.ng:
        length[-1] = f.l_last                                  # whatever its stored scaled length says
    if (width > 32).any():
        raise GribError(f"a group width of {int(width.max())} bits: the widths of the groups go up to 32")
    if int(length.sum()) != f.count:
        raise GribError(f"the group lengths sum to {int(length.sum())}, the field has {f.count} values")
    if at_values + int((length * width).sum()) > bits.size:
        raise GribError(f"the values need {int((length * width).sum())} bits, the stream holds {bits.size - at_values} after its group tables")
    first = np.cumsum(length) - length                         # the first value of a group
    first_bit = at_values + np.cumsum(length * width) - length * width
    group = np.repeat(g, length)                               # the group of value k
    k = np.arange(f.count, dtype=np.int64)
    value_width = width[group]
    start = first_bit[group] + (k - first[group]) * value_width
    X = ref[group].copy()
    for w in np.unique(value_width):
        mine = value_width == w
        X[mine] += _integers_at(bits, start[mine], int(w))
    if f.order == 0:
        return X.view(np.int64)
    wrap = lambda v: np.array([v % 2 ** 64], dtype=np.uint64)   # noqa: E731
    d = X + wrap(f.gmin)
    d[:f.order] = 0                                            # the first `order` values of the stream are placeholders
    if f.order == 1:                                           # f[k] = f[k-1] + d[k]
        return (wrap(f.ival1) + np.cumsum(d, dtype=np.uint64)).view(np.int64)
    # order 2: the first differences g[k] = f[k] - f[k-1] obey g[1] = ival2 - ival1, g[k] = g[k-1] + d[k]; then f[k] = f[k-1] + g[k]
    steps = wrap(f.ival2 - f.ival1) + np.cumsum(d, dtype=np.uint64)
    steps[:1] = 0
    return (wrap(f.ival1) + np.cumsum(steps, dtype=np.uint64)).view(np.int64)


def unpack_fields(fields: Sequence, flip=False) -> List[np.ndarray]:
    """The contract of csrc/grib_unpack.hip (``PackedField``) and csrc/grib_complex.hip (``ComplexField``) in numpy -> one (nj, ni)
    float32 plane per field.  The k-th present point takes the k-th value X of the stream (f[k] of ``complex_integers`` for a
    ComplexField); Y = (R + ldexp(X, E)) / 10^D (``* 10^-D`` for D < 0) in float64, rounded to float32; an absent point, and a present
    one of rank >= count, is NaN.  ``flip`` (one bool, or one per field): stream row r becomes plane row nj-1-r.  A ComplexField whose
    stream contradicts its header (the conditions of the device's status word) raises GribError."""
    flips = [bool(flip)] * len(fields) if isinstance(flip, (bool, np.bool_)) else [bool(f) for f in flip]
    if len(flips) != len(fields):
        raise ValueError(f"{len(flips)} flip flags for {len(fields)} fields")
    out = []
    for f, fl in zip(fields, flips):
        points = f.ni * f.nj
        if f.bitmap is None:
            present = np.ones(points, dtype=bool)
        else:
            present = np.unpackbits(np.frombuffer(f.bitmap, dtype=np.uint8), count=points).astype(bool)
        where = np.flatnonzero(present)[:f.count]           # ranks past count stay NaN
        n = min(f.count, where.size)
        if isinstance(f, ComplexField):
            X = complex_integers(f)[:n].astype(np.float64)
        else:
            X = unpack_bits(bytes(f.stream[:(n * f.nbits + 7) // 8]), n, f.nbits).astype(np.float64) if f.nbits and n else np.zeros(n)
        with np.errstate(all="ignore"):
            scaled = float(f.R) + np.ldexp(X, f.E)
            y = scaled / float(10 ** f.D) if f.D >= 0 else scaled * float(10 ** -f.D)
            plane = np.full(points, np.nan, dtype=np.float32)
            plane[where[:n]] = y.astype(np.float32)
        plane = plane.reshape(f.nj, f.ni)
        out.append(np.ascontiguousarray(plane[::-1]) if fl else plane)
    return out


def window_qualifies(field) -> bool:
    """a simple-packed field without a bitmap: value p lies at bit p * nbits, so a window of it can be decoded on its own"""
    return isinstance(field, PackedField) and field.bitmap is None


def window_slice(field: PackedField, row0: int, row1: int) -> Tuple[int, int, int]:
    """The smallest byte range of ``field.stream`` that holds the NORTH-FIRST plane rows row0 .. row1 - 1 in file order, its start
    rounded down to a multiple of 4 bytes -> (byte_start, byte_end, bit0), ``bit0 = 8 * byte_start`` the bit offset of the slice's
    first byte within the stream.  A file that scans south to north holds plane row r as stream row nj - 1 - r.  Only a field
    ``window_qualifies`` accepts has such a slice; 0 bits per value: the empty slice."""
    if not window_qualifies(field):
        raise GribError("window_slice: only a simple-packed field without a bitmap is random access")
    if not 0 <= row0 < row1 <= field.nj:
        raise GribError(f"window_slice: rows {row0} .. {row1} of a grid of {field.nj} rows")
    first, end = (field.nj - row1, field.nj - row0) if field.south_to_north else (row0, row1)
    if field.nbits == 0:
        return 0, 0, 0
    start = (first * field.ni * field.nbits) // 8 // 4 * 4
    stop = min((end * field.ni * field.nbits + 7) // 8, len(field.stream))
    return start, stop, 8 * start


def unpack_window(field: PackedField, window: Sequence[int], mean: float = 0.0, std: float = 1.0, data=None, bit0: int = 0) -> np.ndarray:
    """The contract of csrc/grib_window.hip for one field in numpy -> (r1 - r0, c1 - c0) float32.  ``window`` = (r0, r1, c0, c1), ends
    exclusive, in NORTH-FIRST plane coordinates (a south-to-north file holds plane row r as stream row nj - 1 - r).  X is the
    nbits-bit big-endian integer at bit (row * ni + col) * nbits - bit0 of ``data``, the shipped slice (default: the whole stream,
    bit0 = 0); v = float32((R + ldexp(X, E)) / 10^D) in float64 (``* 10^-D`` for D < 0); then c = v - mean, c / std in float32."""
    if not window_qualifies(field):
        raise GribError("unpack_window: only a simple-packed field without a bitmap is random access")
    r0, r1, c0, c1 = (int(v) for v in window)
    if not (0 <= r0 < r1 <= field.nj and 0 <= c0 < c1 <= field.ni):
        raise GribError(f"unpack_window: window {tuple(window)} on a grid of {field.nj} x {field.ni}")
    rows = np.arange(r0, r1, dtype=np.int64)
    rows = field.nj - 1 - rows if field.south_to_north else rows
    starts = ((rows[:, None] * field.ni + np.arange(c0, c1, dtype=np.int64)[None, :]) * field.nbits - int(bit0)).reshape(-1)
    if field.nbits:
        bits = np.unpackbits(np.frombuffer(field.stream if data is None else data, dtype=np.uint8))
        if starts.min() < 0 or starts.max() + field.nbits > bits.size:
            raise GribError(f"unpack_window: the window's bits {int(starts.min())} .. {int(starts.max()) + field.nbits} leave the "
                            f"{bits.size // 8} octets given")
        X = _integers_at(bits, starts, field.nbits).astype(np.float64)
    else:
        X = np.zeros(starts.size)
    f4 = np.float32
    with np.errstate(all="ignore"):
        scaled = float(field.R) + np.ldexp(X, field.E)
        v = (scaled / float(10 ** field.D) if field.D >= 0 else scaled * float(10 ** -field.D)).astype(f4)
        c = v - f4(mean)
        return (c / f4(std)).reshape(r1 - r0, c1 - c0)


class GribFile:
    """An index over the messages of one GRIB2 file for reading: ``find(fid)`` matches as ``Template.find`` does (numeric
    MATCHED_KEYS only, no ``shortName``), ``field(fid)`` is ``field_of`` of that message -- ``complex_field_of`` for templates 5.2 and
    5.3 -- parsed once."""

    def __init__(self, path):
        self.path = path
        self.messages = read_messages(path)
        if not self.messages:
            raise GribError(f"{path}: no GRIB2 message")
        self._fields: Dict[int, object] = {}

    def find(self, fid: dict) -> Message:
        if not set(fid) - set(IGNORED_KEYS):
            raise GribError(f"{self.path}: keys {sorted(fid)} hold none of {MATCHED_KEYS}: matching by shortName (eccodes' tables) is "
                            f"out of scope, messages are found by their numeric keys")
        return find_message(self.messages, fid, self.path)

    def field(self, fid: dict) -> Tuple[Message, object]:
        m = self.find(fid)
        if id(m) not in self._fields:
            try:
                complex_packed = m.keys["dataRepresentationTemplateNumber"] in COMPLEX_TEMPLATES
                self._fields[id(m)] = complex_field_of(m) if complex_packed else field_of(m)
            except GribError as e:
                raise GribError(f"{self.path}: {e}") from None
        return m, self._fields[id(m)]


# ------------------------------------------------------------------------------------------------ the packer on the CPU
def _quantise(v: np.ndarray, D: int, nbits: int):
    """the quantisation of csrc/grib_pack.hip: v fp32 (N,) -> (vmin, vmax, R, E, bad, X uint64)"""
    if abs(D) > MAX_D or not 1 <= nbits <= 32:
        raise GribError(f"D = {D}, nbits = {nbits}: |D| <= {MAX_D} and 1 <= nbits <= 32 are packed")
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    finite = np.isfinite(v)
    bad = int(v.size - finite.sum())
    pw = float(10 ** abs(D))
    with np.errstate(all="ignore"):
        s = v.astype(np.float64) * pw if D >= 0 else v.astype(np.float64) / pw
    xmax = float(2 ** nbits - 1)
    if bad == v.size:
        vmin = vmax = np.float32(np.nan)
        R, E = np.float32(0.0), 0
    else:
        vmin, vmax = v[finite].min(), v[finite].max()
        smin, smax = (float(x) * pw if D >= 0 else float(x) / pw for x in (vmin, vmax))
        with np.errstate(all="ignore"):
            R = np.float32(smin)
        if float(R) > smin:
            R = np.nextafter(R, np.float32(-np.inf))
        E, span = 0, smax - float(R)
        if vmax != vmin and 0.0 < span < math.inf:
            E = math.frexp(span)[1] - nbits - 1
            while math.ldexp(span, -E) > xmax:
                E += 1
    with np.errstate(all="ignore"):
        X = np.floor(np.ldexp(s - float(R), -E) + 0.5)
        X = np.where(X < xmax, np.where(X > 0.0, X, 0.0), xmax).astype(np.uint64)
    return vmin, vmax, R, E, bad, X


def pack_simple(v: np.ndarray, D: int, nbits: int):
    """The contract of csrc/grib_pack.hip for one field in stream order: v fp32 (N,) -> (vmin, vmax, R, E, bad, the stream's bytes)"""
    vmin, vmax, R, E, bad, X = _quantise(v, D, nbits)
    bits = ((X[:, None] >> np.arange(nbits - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    return vmin, vmax, R, E, bad, np.packbits(bits.reshape(-1)).tobytes()


def _bit_lengths(a: np.ndarray) -> np.ndarray:
    """the bit length of every element of a non-negative int64 array below 2^33"""
    out = np.zeros(a.shape, dtype=np.int64)
    for b in range(33):
        out[a >= (1 << b)] = b + 1
    return out


def _table_bits(values: np.ndarray, width: int) -> np.ndarray:
    """the integers ``values`` in ``width`` bits each, most significant bit first, zero-padded to an octet -> 0/1 uint8"""
    if width == 0 or values.size == 0:
        return np.zeros(0, dtype=np.uint8)
    v = values.astype(np.uint64)
    bits = ((v[:, None] >> np.arange(width - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).reshape(-1)
    return np.concatenate([bits, np.zeros(-bits.size % 8, dtype=np.uint8)])


def pack_complex(v: np.ndarray, D: int, nbits: int, order: int):
    """The contract of csrc/grib_pack_complex.hip for one field in stream order: v fp32 (N,) -> (vmin, vmax, R, E, bad, numbers,
    payload).  X is that of ``pack_simple``; order 0: d = X; 1: d[q] = X[q] - X[q-1]; 2: d[q] = X[q] - 2 X[q-1] + X[q-2]; gmin the
    minimum of d over q >= order (0 at order 0 or without such a q); X' = d - gmin, 0 for q < order.  Groups of 32 values, the last one
    shorter: reference min X', width the bits of max X' - min X'.  ``numbers``: ival1 = X[0], ival2 = X[1] (order 2), gmin, ref_bits
    (the bits of the largest reference), ng, l_last.  ``payload``: the descriptors (order >= 1: ival1, [ival2,] gmin in 4 octets each,
    sign and magnitude), the references in ref_bits bits, the widths in 6, the values X' - reference in their group's width, each part
    zero-padded to an octet; empty for a field with bad > 0."""
    check_complex(nbits, order)
    vmin, vmax, R, E, bad, X = _quantise(v, D, nbits)
    N = X.size
    f = X.astype(np.int64)
    d = f.copy()
    if order == 1:
        d[1:] = f[1:] - f[:-1]
    elif order == 2:
        d[2:] = f[2:] - 2 * f[1:-1] + f[:-2]
    gmin = int(d[order:].min()) if order and N > order else 0
    Xp = d - gmin
    Xp[:order] = 0
    starts = np.arange(0, N, COMPLEX_GROUP)
    ng = starts.size
    ref = np.minimum.reduceat(Xp, starts)
    width = _bit_lengths(np.maximum.reduceat(Xp, starts) - ref)
    ref_bits = int(_bit_lengths(ref.max(keepdims=True))[0])
    numbers = dict(ival1=int(f[0]) if order else 0, ival2=int(f[1]) if order == 2 and N > 1 else 0, gmin=gmin, ref_bits=ref_bits, ng=ng,
                   l_last=N - COMPLEX_GROUP * (ng - 1))
    if bad:
        return vmin, vmax, R, E, bad, numbers, b""
    head = bytearray()
    if order:
        for value in ([numbers["ival1"], numbers["ival2"], gmin] if order == 2 else [numbers["ival1"], gmin]):
            b = bytearray(4)
            _put_s(b, 1, 4, value)
            head += b
    group = np.arange(N) // COMPLEX_GROUP
    rest, wide = (Xp - ref[group]).astype(np.uint64), width[group]
    length = np.diff(np.append(starts, N))
    group_bits = length * width
    first_bit = np.cumsum(group_bits) - group_bits                     # of a group: a multiple of 8, a full group is 4 w octets
    at = first_bit[group] + (np.arange(N) - starts[group]) * wide
    bits = np.zeros((int(group_bits.sum()) + 7) // 8 * 8, dtype=np.uint8)
    for w in np.unique(wide):
        if w:
            mine = wide == w
            idx = at[mine][:, None] + np.arange(w, dtype=np.int64)
            bits[idx] = ((rest[mine][:, None] >> np.arange(w - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    stream = np.concatenate([_table_bits(ref, ref_bits), _table_bits(width, COMPLEX_W_BITS), bits])
    return vmin, vmax, R, E, bad, numbers, bytes(head) + np.packbits(stream).tobytes()


def pack_fields(pred: np.ndarray, std: np.ndarray, mean: np.ndarray, spec: Sequence[Tuple[int, int]], samples: Sequence[int],
                features: Sequence[int], H: int, W: int, flip_rows: bool, pitch: Optional[int] = None):
    """``ops.grib_pack`` on the CPU: pred (B,T,N,F) fp32 normalised -> params (n,T,K,5) int32, packed (n,T,K,pitch) uint8.  With a
    ``spec`` of (D, nbits, order) triples it is ``ops.grib_pack_complex``: params (n,T,K,11) int32 and one uint8 buffer of the call's
    capacity with the payloads at their offsets, zero elsewhere."""
    pred = np.asarray(pred, dtype=np.float32)
    std, mean = np.asarray(std, dtype=np.float32), np.asarray(mean, dtype=np.float32)
    n, T, K = len(samples), pred.shape[1], len(features)
    if len(spec) and len(spec[0]) == 3:
        params = np.zeros((n, T, K, COMPLEX_PARAMS), dtype=np.int32)
        out = np.zeros(n * T * sum(complex_capacity(H * W, nbits, order) for _, nbits, order in spec), dtype=np.uint8)
        at = 0
        for i, b in enumerate(samples):
            for t in range(T):
                for k, f in enumerate(features):
                    a = pred[b, t, :, f] * std[f]
                    v = (a + mean[f]).astype(np.float32).reshape(H, W)
                    vmin, vmax, R, E, bad, nm, payload = pack_complex(v[::-1] if flip_rows else v, *spec[k])
                    params[i, t, k, :3] = np.array([vmin, vmax, R], dtype=np.float32).view(np.int32)
                    params[i, t, k, 3:] = (E, bad, nm["ival1"], nm["ival2"], nm["gmin"], nm["ref_bits"], len(payload), at)
                    out[at:at + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
                    at += (len(payload) + 3) // 4 * 4
        return params, out
    params = np.zeros((n, T, K, 5), dtype=np.int32)
    packed = np.zeros((n, T, K, pitch), dtype=np.uint8)
    for i, b in enumerate(samples):
        for t in range(T):
            for k, f in enumerate(features):
                a = pred[b, t, :, f] * std[f]
                v = (a + mean[f]).astype(np.float32).reshape(H, W)
                if flip_rows:
                    v = v[::-1]
                vmin, vmax, R, E, bad, stream = pack_simple(v, spec[k][0], spec[k][1])
                params[i, t, k, :3] = np.array([vmin, vmax, R], dtype=np.float32).view(np.int32)
                params[i, t, k, 3:] = (E, bad)
                packed[i, t, k, :len(stream)] = np.frombuffer(stream, dtype=np.uint8)
    return params, packed
