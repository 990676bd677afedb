"""Generated forcings, the parts that need no GPU: the float64 closed form against the reference's golden arrays (within the
reference's own stored deviation), the reference's two known answers, the host tables of ``py4cast_amd.forcings`` and the
feature names."""

import datetime as dt
import os

import numpy as np
import pytest
import torch

import forcing_closed_form as cf

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = ["case0", "case1", "case2"]


def _load(name):
    z = np.load(os.path.join(GOLD, f"forcing_{name}.npz"))
    return z, cf.to_dates(z["dates"]), cf.to_terms(z["term_seconds"])


@pytest.mark.parametrize("name", CASES + ["known"])
def test_closed_form_reproduces_reference(name):
    z, dates, terms = _load(name)
    want_date, cos_sza, want_toa = cf.batch(z["lat"], z["lon"], dates, terms)
    assert z["lat"].dtype == np.float32 and z["lon"].dtype == np.float32
    assert z["ref_date"].shape == want_date.shape and z["ref_toa"].shape == want_toa.shape + (1,)
    d_date, d_toa = np.abs(z["ref_date"] - want_date).max(), np.abs(z["ref_toa"][..., 0] - want_toa).max()
    print(f"{name}: date {d_date:.3g} (stored {float(z['d_ref_date']):.3g}), toa {d_toa:.3g} (stored {float(z['d_ref_toa']):.3g})")
    assert d_date <= float(z["d_ref_date"]) and d_toa <= float(z["d_ref_toa"])
    assert float(z["d_ref_toa"]) < 0.01   # the reference's own margin (its tests/test_datasets.py:152)
    if name != "known":     # a case without night, or without day, checks nothing
        assert (z["ref_toa"] > 1.0).any() and (cos_sza < -1e-3).any() and (z["ref_toa"][cos_sza < -1e-6] == 0).all()


def test_known_answers():
    """the reference's own two (its tests/test_datasets.py:114-161): midnight of the new year 2024, and exercise 1.6.2.a of
    Solar Engineering of Thermal Processes (zenith angle 66.5 degrees at latitude 43, 9:30 solar time on 13 February)"""
    from py4cast_amd import forcings

    date, terms = dt.datetime(2023, 12, 31, 23), [dt.timedelta(hours=1)]
    z, dates, all_terms = _load("case0")
    assert dates[0] == date and all_terms[0] == terms[0]
    for got in (cf.date_values(date, terms)[0], z["ref_date"][0, 0], forcings.time_table([date], terms)[0, 0, :4].numpy()):
        np.testing.assert_allclose(got, [0.5, 1, 0.5, 1], rtol=1e-5, atol=1e-8)     # torch.allclose's defaults, as the reference's test
    z, dates, terms = _load("known")
    assert dates == [dt.datetime(2023, 2, 13, 15, 26)] and z["lat"].item() == 43 and z["lon"].item() == -89
    solution = 1366 * np.cos(np.radians(66.5))
    assert abs(z["ref_toa"].item() - solution) < 0.01
    assert abs(cf.toa(z["lat"], z["lon"], dates[0], terms).item() - solution) < 0.01
    # the same through the host tables, in float64: what the kernel evaluates in fp32
    e = forcings.time_table(dates, terms)[0, 0].double().numpy()
    s, c, lh = forcings.grid_tables(z["lat"], z["lon"], "cpu").double().numpy().reshape(3)
    assert abs(1366 * (s * e[4] + c * e[5] * np.cos(np.radians(15 * (e[6] + lh - 12)))) - solution) < 0.01


@pytest.mark.parametrize("name", CASES)
def test_time_table_within_d_ref_of_reference(name):
    """|time_table - reference's date forcing| <= d_ref_date.  The nearest fp32 of the float64 value does NOT meet this (case1:
    1.192e-07 against 1.065e-07, case2: 2.682e-07 against 2.678e-07: it lies on the other side of the true value from the
    reference), which is why the date columns are evaluated with the reference's fp32 operations."""
    from py4cast_amd import forcings

    z, dates, terms = _load(name)
    d = np.abs(forcings.time_table(dates, terms)[..., :4].double().numpy() - z["ref_date"]).max()
    print(f"{name}: time_table against the reference's date forcing {d:.3g}, d_ref_date {float(z['d_ref_date']):.3g}")
    assert d <= float(z["d_ref_date"])


@pytest.mark.parametrize("name", CASES)
def test_time_table_against_closed_form(name):
    """date columns: within the reference's own deviation of the float64 closed form plus the one fp32 step (values in [0, 1]:
    2**-24) that another build of the sine and cosine may move a value by; sin(dec), cos(dec) and the hour: the float64 value
    rounded once"""
    from py4cast_amd import forcings

    z, dates, terms = _load(name)
    table = forcings.time_table(dates, terms)
    assert table.shape == (len(dates), len(terms), 8) and table.dtype == torch.float32 and (table[..., 7] == 0).all()
    t = table.numpy()
    want = np.stack([cf.date_values(x, terms) for x in dates])
    assert np.abs(t[..., :4] - want).max() <= float(z["d_ref_date"]) + 2.0 ** -24
    dec = np.stack([cf.declination(x, terms) for x in dates])
    hours = np.stack([cf.hours_of_day(x, terms) for x in dates])
    for got, want in ((t[..., 4], np.sin(dec)), (t[..., 5], np.cos(dec)), (t[..., 6], hours)):
        np.testing.assert_allclose(got, want, rtol=2.0 ** -24, atol=0)


def test_time_table_conventions():
    """each of the reference's conventions moves a value by far more than rounding"""
    from py4cast_amd import forcings

    h = dt.timedelta(hours=1)
    # seconds count from 1 January of date.year: across the new year the angle runs past 2 pi and stays continuous
    t = forcings.time_table([dt.datetime(2023, 12, 31, 23)], [0 * h, 1 * h, 2 * h]).double().numpy()[0]
    year_angle = np.arctan2(2 * t[:, 2] - 1, 2 * t[:, 3] - 1)
    # the angle is an fp32 value near 2 pi (step 4.8e-07) and so are its sine and cosine: a few steps against an hour's 7.2e-04;
    # an angle that restarted at the new year would jump by 2 pi
    np.testing.assert_allclose(np.diff(year_angle), 2 * np.pi / (365 * 24), rtol=0, atol=4 * 4.8e-07)
    # the day of year is taken from date + term and starts at 1
    dec = np.degrees(np.arcsin(t[:, 4]))
    np.testing.assert_allclose(dec, 23.45 * np.sin(2 * np.pi * (284 + np.array([365, 1, 1])) / 365), atol=1e-4)
    # a leap year has 366 days: half of it ends at noon of 2 July
    t = forcings.time_table([dt.datetime(2024, 1, 1)], [dt.timedelta(days=183)])[0, 0]
    np.testing.assert_allclose(t[2:4].numpy(), [0.5, 0.0], atol=1e-7)
    # minutes count, seconds do not
    assert float(forcings.time_table([dt.datetime(2024, 2, 29, 5, 30, 59)], [0 * h])[0, 0, 6]) == 5.5


def test_grid_tables_and_cache():
    from py4cast_amd import forcings

    z, _, _ = _load("case1")
    lat, lon = torch.from_numpy(z["lat"]), torch.from_numpy(z["lon"])
    planes = forcings.grid_tables(lat, lon, "cpu")
    assert planes.shape == (3,) + lat.shape and planes.dtype == torch.float32 and planes.is_contiguous()
    want = np.stack([np.sin(np.radians(z["lat"].astype(np.float64))), np.cos(np.radians(z["lat"].astype(np.float64))), z["lon"].astype(np.float64) / 15])
    assert np.array_equal(planes.numpy(), want.astype(np.float32))
    assert forcings.grid_tables(lat, lon, "cpu") is planes                     # same grid, same device: the cached planes
    assert forcings.grid_tables(z["lat"].astype(np.float64), z["lon"], "cpu") is not planes
    assert torch.equal(forcings.grid_tables(z["lat"].astype(np.float64), z["lon"], "cpu"), planes)  # float64 input: rounded to fp32 first
    lat.add_(1.0)                                                                # an in-place change is seen
    assert not torch.equal(forcings.grid_tables(lat, lon, "cpu"), planes)
    with pytest.raises(ValueError):
        forcings.grid_tables(lat, lon[:, :-1], "cpu")
    with pytest.raises(ValueError):
        forcings.grid_tables(lat[0], lon[0], "cpu")


@pytest.mark.parametrize("name", CASES)
def test_host_forcing_against_closed_form(name):
    """the host statement of the kernel's arithmetic (float64 on the fp32 tables): within the reference's own deviation of the
    closed form, zero at night, date values the table's"""
    from py4cast_amd import forcings

    z, dates, terms = _load(name)
    got = forcings.host_forcing(dates, terms, z["lat"], z["lon"])
    assert got.shape == (len(dates), len(terms)) + z["lat"].shape + (5,) and got.dtype == torch.float32
    _, cos_sza, want_toa = cf.batch(z["lat"], z["lon"], dates, terms)
    assert np.abs(got[..., 4].double().numpy() - want_toa).max() <= float(z["d_ref_toa"])
    assert (got[..., 4].numpy()[cos_sza < -1e-6] == 0).all()
    assert torch.equal(got[..., :4], forcings.time_table(dates, terms)[:, :, None, None, :4].expand(got.shape[:-1] + (4,)))


def test_feature_names_are_the_references():
    from py4cast_amd import forcings

    assert forcings.FORCING_NAMES == ["cos_hour", "sin_hour", "cos_doy", "sin_doy", "toa_radiation"] == cf.NAMES


def test_build_forcing_has_no_cpu_path():
    from py4cast_amd import _lib, forcings, ops

    table = forcings.time_table([dt.datetime(2023, 3, 20, 11)], [dt.timedelta(hours=1)])
    planes = forcings.grid_tables(torch.zeros(4, 4), torch.zeros(4, 4), "cpu")
    with pytest.raises(_lib.P4CError):
        ops.build_forcing(None, None, None, table, planes, 1, 1, 4, 4)
    with pytest.raises(_lib.P4CError):
        ops.build_forcing(torch.zeros(2, 1, 1, 4, 4), torch.zeros(2), torch.ones(2), table, planes, 1, 1, 4, 4)
