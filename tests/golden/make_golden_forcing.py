#!/usr/bin/env python3
"""
Golden vectors for the generated forcings -- runs ONLY in the build container (needs the reference).

Imports the reference's unmodified ``py4cast/forcingutils.py`` (numpy and torch only, no stubs needed) and calls
``get_year_hour_forcing`` and ``generate_toa_radiation_forcing`` per run date, as ``generate_forcings`` does
(datasets/base.py:233-274, both results cast to float32).  Per case it stores the fp32 coordinates, the dates and lead
times as integers, the reference's arrays, and ``d_ref_date`` / ``d_ref_toa``: the reference's own worst absolute
deviation from the float64 closed form (tests/forcing_closed_form.py) on the same fp32-rounded coordinates -- the unit
the tests' tolerances are counted in.

Every case must hold lit and dark pixels (an all-night case checks nothing: 2023-12-31 23:00 + 1..3 h over Europe is
entirely zero).

    python tests/golden/make_golden_forcing.py
"""

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import forcing_closed_form as cf  # noqa: E402
import make_golden as mg  # noqa: E402  (where the reference lies)


def load_reference():
    spec = importlib.util.spec_from_file_location("py4cast_forcingutils", os.path.join(mg.REF, "py4cast", "forcingutils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)   # unmodified reference file
    return mod


def grid(lat0, lat1, lon0, lon1, H, W):
    lat, lon = np.meshgrid(np.linspace(lat1, lat0, H), np.linspace(lon0, lon1, W), indexing="ij")
    return lat.astype(np.float32), lon.astype(np.float32)


def gen_case(fu, name, lat, lon, dates, term_seconds, need_dark=True):
    dts, terms = cf.to_dates(dates), cf.to_terms(term_seconds)
    lat_t, lon_t = torch.from_numpy(lat), torch.from_numpy(lon)
    ref_date = torch.stack([fu.get_year_hour_forcing(d, terms).type(torch.float32) for d in dts]).numpy()
    ref_toa = torch.stack([fu.generate_toa_radiation_forcing(lat_t, lon_t, d, terms).type(torch.float32) for d in dts]).numpy()
    B, T = len(dts), len(terms)
    assert ref_date.shape == (B, T, 4) and ref_toa.shape == (B, T) + lat.shape + (1,), (ref_date.shape, ref_toa.shape)
    assert ref_date.dtype == np.float32 and ref_toa.dtype == np.float32
    want_date, cos_sza, want_toa = cf.batch(lat, lon, dts, terms)
    d_ref_date = float(np.abs(ref_date - want_date).max())
    d_ref_toa = float(np.abs(ref_toa[..., 0] - want_toa).max())
    lit, dark = int((ref_toa > 1.0).sum()), int((cos_sza < -1e-3).sum())
    if need_dark:
        assert lit > 0 and dark > 0, f"{name}: {lit} lit and {dark} dark pixels: the case must hold both"
    assert d_ref_toa < 0.01, d_ref_toa
    path = os.path.join(HERE, f"forcing_{name}.npz")
    np.savez_compressed(path, lat=lat, lon=lon, dates=np.asarray(dates, dtype=np.int64), term_seconds=np.asarray(term_seconds, dtype=np.int64),
                        ref_date=ref_date, ref_toa=ref_toa, d_ref_date=np.float64(d_ref_date), d_ref_toa=np.float64(d_ref_toa))
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, lit {lit}, dark {dark}, d_ref_date {d_ref_date:.3g}, d_ref_toa {d_ref_toa:.3g}")


if __name__ == "__main__":
    fu = load_reference()
    h = 3600
    # both hemispheres, hour angle beyond +-180 degrees; new-year crossing; leap year with fractional hours
    gen_case(fu, "case0", *grid(-89, 89, -180, 180, 17, 19), [[2023, 12, 31, 23, 0], [2024, 2, 29, 5, 30]], [1 * h, 2 * h, 3 * h])
    # Europe-like; the March date sits at the equinox, where one day of doy moves lit pixels by several W/m2
    gen_case(fu, "case1", *grid(37, 55, -12, 16, 24, 40), [[2023, 3, 20, 11, 15], [2023, 6, 21, 11, 15]], [1 * h, 6 * h + 1800])
    gen_case(fu, "case2", *grid(-60, 60, -170, 170, 8, 8), [[2022, 8, 15, 14, 20]], [3 * h])
    # the reference's own known answer (its tests/test_datasets.py:136-161): exercise 1.6.2.a of Solar Engineering of Thermal
    # Processes: latitude 43, longitude -89, 13 February 9:30 solar time = 15:26 UTC -> zenith angle 66.5 degrees
    gen_case(fu, "known", np.full((1, 1), 43, np.float32), np.full((1, 1), -89, np.float32), [[2023, 2, 13, 15, 26]], [0], need_dark=False)
