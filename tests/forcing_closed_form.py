"""float64 numpy statement of the reference's generated forcings (py4cast/forcingutils.py:19-132, assembled by
``generate_forcings``, datasets/base.py:233-274), shared by the forcing tests and the golden generator.  Written from the
formulas, independent of py4cast_amd:

date values   (sin, cos) of the hour angle 2 pi hour / 24 and (sin, cos) of the year angle 2 pi seconds / seconds_in_year,
              each rescaled (v + 1) / 2.  hour = hour + minute / 60 of date + term; seconds count from 1 January of
              date.year (NOT of (date + term).year); the year has 366 days if date.year % 4 == 0 else 365.
irradiance    1366 * max(0, cos_sza), cos_sza = sin(phi) sin(dec) + cos(phi) cos(dec) cos(omega), omega = 15 deg * (hour +
              lon / 15 - 12), dec = 23.45 deg * sin(2 pi (284 + doy) / 365) with doy counted from 1 on date + term."""

import datetime as dt

import numpy as np

E0 = 1366.0
NAMES = ["cos_hour", "sin_hour", "cos_doy", "sin_doy", "toa_radiation"]   # base.py:249-271, in concatenation order


def to_dates(rows):
    """(B, 5) integers year, month, day, hour, minute -> datetimes"""
    return [dt.datetime(*(int(v) for v in r)) for r in np.asarray(rows)]


def to_terms(seconds):
    return [dt.timedelta(seconds=int(s)) for s in np.asarray(seconds)]


def hours_of_day(date, terms):
    return np.array([(date + t).hour + (date + t).minute / 60 for t in terms], dtype=np.float64)


def days_of_year(date, terms):
    return np.array([((date + t) - dt.datetime((date + t).year, 1, 1)).days + 1 for t in terms], dtype=np.float64)


def declination(date, terms):
    """radians, (T,)"""
    return np.radians(23.45 * np.sin(2 * np.pi * (284 + days_of_year(date, terms)) / 365))


def date_values(date, terms):
    """(T, 4) float64"""
    hour_angle = hours_of_day(date, terms) / 12 * np.pi
    seconds = np.array([(date + t - dt.datetime(date.year, 1, 1)).total_seconds() for t in terms], dtype=np.float64)
    year_angle = seconds / ((366 if date.year % 4 == 0 else 365) * 86400) * 2 * np.pi
    return (np.stack([np.sin(hour_angle), np.cos(hour_angle), np.sin(year_angle), np.cos(year_angle)], axis=1) + 1) / 2


def cos_zenith(lat, lon, date, terms):
    """lat, lon (H, W) degrees (taken as they are, in float64) -> (T, H, W) float64"""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    omega = np.radians(15 * (hours_of_day(date, terms)[:, None, None] + lon / 15 - 12))
    dec = declination(date, terms)[:, None, None]
    phi = np.radians(lat)
    return np.sin(phi) * np.sin(dec) + np.cos(phi) * np.cos(dec) * np.cos(omega)


def toa(lat, lon, date, terms):
    return np.maximum(0.0, E0 * cos_zenith(lat, lon, date, terms))


def batch(lat, lon, dates, terms):
    """-> date values (B, T, 4), cos_sza (B, T, H, W), irradiance (B, T, H, W), float64"""
    d = np.stack([date_values(x, terms) for x in dates])
    c = np.stack([cos_zenith(lat, lon, x, terms) for x in dates])
    return d, c, np.maximum(0.0, E0 * c)
