"""
Host side of the generated forcings: the reference appends five channels of its own to every sample's
forcing tensor (``generate_forcings``, datasets/base.py:233-274, calling py4cast/forcingutils.py): four date values and the
top-of-atmosphere solar irradiance.  The kernel ``p4c_build_forcing`` computes them per pixel from two small tables built
here: one entry per (sample, lead time) and three planes per grid.  What feeds the kernel's arithmetic is evaluated in float64
and rounded once; the four date values, which the kernel only copies, are evaluated as the reference evaluates them.
"""

import datetime as dt
import math
from collections import OrderedDict
from typing import Sequence

import torch

# The reference's names in the reference's order (base.py:249-271).  The values under "cos_hour" / "sin_hour" really are the
# SINE then the COSINE of the hour angle, and likewise for the year angle (get_year_hour_forcing stacks sin, cos, sin, cos;
# base.py:250-263 labels the columns cos, sin).  Trained weights and statistics files carry these names: the quirk is kept.
FORCING_NAMES = ["cos_hour", "sin_hour", "cos_doy", "sin_doy", "toa_radiation"]

TABLE_WIDTH = 8  # floats per (sample, lead time): 4 date values, sin and cos of the declination, UTC hour, one pad


def time_table(dates: Sequence[dt.datetime], timedeltas: Sequence[dt.timedelta]) -> torch.Tensor:
    """(B, T, 8) fp32 for B run dates and T lead times, with the reference's conventions (forcingutils.py:19-132):

    * hour of day = hour + minute / 60 of ``date + term`` (seconds are dropped);
    * the year angle counts seconds from 1 January of ``date.year`` -- not of ``(date + term).year`` -- over a year of
      366 days if ``date.year % 4 == 0`` else 365: across a new year it runs past 2 pi;
    * columns 0-3: (sin, cos) of the hour angle, (sin, cos) of the year angle, each rescaled ``(v + 1) / 2``;
    * the day of year counts from 1 and IS taken from ``date + term``; declination 23.45 deg * sin(2 pi (284 + doy) / 365),
      365 always; columns 4-5 its sine and cosine, column 6 the hour of day, column 7 zero.

    Columns 4-6 feed the kernel's arithmetic: float64, rounded once.  Columns 0-3 ARE the output channels, so they are
    evaluated as the reference evaluates them (``_date_values``): the nearest fp32 of the float64 value lies up to two fp32 steps
    from what the reference hands a model (it sits on the other side of the true value), the same fp32 operations reproduce it."""
    date_values, rest = [], []
    for date in dates:
        start = dt.datetime(date.year, 1, 1, tzinfo=date.tzinfo)
        whens = [date + term for term in timedeltas]
        hours = [w.hour + w.minute / 60 for w in whens]
        seconds = [(w - start).total_seconds() for w in whens]
        date_values.append(_date_values(hours, seconds, 366 if date.year % 4 == 0 else 365))
        for w, hour in zip(whens, hours):
            doy = (w - dt.datetime(w.year, 1, 1, tzinfo=w.tzinfo)).days + 1
            dec = math.radians(23.45 * math.sin(2 * math.pi * (284 + doy) / 365))
            rest.append((math.sin(dec), math.cos(dec), hour, 0.0))
    rest = torch.tensor(rest, dtype=torch.float64).float().view(len(dates), len(timedeltas), TABLE_WIDTH - 4)
    return torch.cat([torch.stack(date_values), rest], dim=-1)


def _date_values(hours, seconds, days_in_year: int) -> torch.Tensor:
    """(T, 4) fp32 for one run date: the reference's own sequence of fp32 tensor operations (get_year_hour_forcing,
    forcingutils.py:61-87: hours and seconds rounded to fp32 first, every step one fp32 operation on a (T,) tensor), so that the
    channels are the values the reference produces rather than values 1e-7 beside them."""
    hour_angle = torch.tensor(hours, dtype=torch.float64).float() / 12 * torch.pi
    year_angle = torch.tensor(seconds, dtype=torch.float64).float() / (days_in_year * 24 * 60 * 60) * 2 * torch.pi
    waves = torch.stack((torch.sin(hour_angle), torch.cos(hour_angle), torch.sin(year_angle), torch.cos(year_angle)), dim=1)
    return (waves + 1) / 2


def host_forcing(dates: Sequence[dt.datetime], timedeltas: Sequence[dt.timedelta], lat, lon) -> torch.Tensor:
    """The five generated channels (B, T, H, W, 5) on the host, in float64 from the same two tables and rounded once to fp32:
    what the reference assembles per sample on the CPU.  For checks and timing comparisons; the pipeline uses the kernel."""
    table = time_table(dates, timedeltas).double()
    sin_lat, cos_lat, lon_hours = _grid_planes(torch.as_tensor(lat), torch.as_tensor(lon)).double()
    e = table[:, :, None, None, :]
    omega = torch.deg2rad(15 * (e[..., 6] + lon_hours - 12))
    toa = torch.clamp_min(1366 * (sin_lat * e[..., 4] + cos_lat * e[..., 5] * torch.cos(omega)), 0)
    date = e[..., :4].expand(toa.shape + (4,))
    return torch.cat([date, toa.unsqueeze(-1)], dim=-1).float()


_GRID_CACHE: "OrderedDict[tuple, tuple]" = OrderedDict()
_GRID_CACHE_SIZE = 8


def _grid_planes(lat: torch.Tensor, lon: torch.Tensor) -> torch.Tensor:
    """(3, H, W) fp32 on the host: sin(lat), cos(lat), lon / 15.  The reference holds its grid in fp32 (``torch.Tensor(lat)``):
    the coordinates are rounded to fp32 first, then evaluated in float64."""
    phi = torch.deg2rad(lat.detach().cpu().float().double())
    hours = lon.detach().cpu().float().double() / 15
    return torch.stack([torch.sin(phi), torch.cos(phi), hours]).float().contiguous()


def grid_tables(lat, lon, device) -> torch.Tensor:
    """The three per-grid planes of ``p4c_build_forcing`` as one (3, H, W) fp32 tensor on ``device``: sine and cosine of the
    latitude and the longitude in hours.  ``lat`` and ``lon`` are (H, W) in degrees, tensors or arrays.

    Cached per (grid, device), the grid identified by the storage of ``lat`` and ``lon`` (which the cache keeps alive) and, for
    tensors, their in-place version counters; an array rewritten in place needs ``grid_tables_clear()``."""
    lat_t, lon_t = torch.as_tensor(lat), torch.as_tensor(lon)
    if lat_t.dim() != 2 or lon_t.shape != lat_t.shape:
        raise ValueError(f"grid_tables: lat {tuple(lat_t.shape)} and lon {tuple(lon_t.shape)} must be the same (H, W)")
    device = torch.device(device)
    if device.type == "cuda" and device.index is None and torch.cuda.is_available():
        device = torch.device("cuda", torch.cuda.current_device())
    key = tuple((t.data_ptr(), t._version, t.dtype, tuple(t.shape), t.stride(), str(t.device)) for t in (lat_t, lon_t)) + (str(device),)
    hit = _GRID_CACHE.get(key)
    if hit is not None:
        _GRID_CACHE.move_to_end(key)
        return hit[0]
    planes = _grid_planes(lat_t, lon_t).to(device)
    _GRID_CACHE[key] = (planes, lat_t, lon_t)
    while len(_GRID_CACHE) > _GRID_CACHE_SIZE:
        _GRID_CACHE.popitem(last=False)
    return planes


def grid_tables_clear():
    _GRID_CACHE.clear()
