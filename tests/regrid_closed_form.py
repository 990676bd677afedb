"""The regrid chain in float64 numpy, written from its formulas (no scipy, nothing of py4cast_amd): the reference the CPU
and GPU tests compare against.  tests/golden/regrid_*.npz pin it to scipy.ndimage.

Per axis, source length n (after the window crop), full target length N:
    x(o) = ((2 o + 1) n - N) / (2 N);   x < 0 -> -x;   x > n - 1 -> 2 (n - 1) - x
    i0 = floor(x), i1 = min(i0 + 1, n - 1), f = x - i0
    blur: sigma = max(0, (n / N - 1) / 2), r = int(4 sigma + 0.5), w_k = exp(-k^2 / (2 sigma^2)) / sum, mirror with period 2 (n - 1)
Chain: window crop -> blur (anti_aliasing) -> resize -> latitude flip -> sub-domain."""

from fractions import Fraction

import numpy as np


def source_field(shape, i0=0, j0=0):
    """an analytic field with structure at every scale the tests resample, float64 evaluated, cast to fp32"""
    i, j = np.meshgrid(np.arange(shape[0], dtype=np.float64) + i0, np.arange(shape[1], dtype=np.float64) + j0, indexing="ij")
    return (np.sin(0.37 * i + 0.002 * j * j) + 0.3 * np.cos(0.11 * j) + 1e-3 * i).astype(np.float32)


def coordinates(n, N, outputs):
    """(i0, i1, f) of the resized-axis indices ``outputs``: exact fractions, f rounded to float64 once"""
    i0, i1, f = [], [], []
    for o in outputs:
        x = Fraction((2 * int(o) + 1) * n - N, 2 * N)
        if x < 0:
            x = -x
        if x > n - 1:
            x = 2 * (n - 1) - x
        lo = x.numerator // x.denominator
        i0.append(lo)
        i1.append(min(lo + 1, n - 1))
        f.append(float(x - lo))
    return np.array(i0), np.array(i1), np.array(f, dtype=np.float64)


def mirror(idx, n):
    p = np.asarray(idx) % (2 * (n - 1))
    return np.where(p > n - 1, 2 * (n - 1) - p, p)


def gaussian(n, N):
    sigma = max(0.0, (n / N - 1) / 2)
    r = int(4 * sigma + 0.5)
    if r == 0:
        return sigma, 0, np.ones(1)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-k * k / (2 * sigma * sigma))
    return sigma, r, w / w.sum()


def blur(img, full_size):
    img = np.asarray(img, dtype=np.float64)
    for axis in (0, 1):
        n = img.shape[axis]
        _, r, w = gaussian(n, full_size[axis])
        if r == 0:
            continue
        acc = np.zeros_like(img)
        for k in range(-r, r + 1):
            acc += w[k + r] * np.take(img, mirror(np.arange(n) + k, n), axis=axis)
        img = acc
    return img


def output_indices(full_size, subdomain, flip_lat):
    a, b, c, d = subdomain if subdomain is not None else (0, full_size[0], 0, full_size[1])
    rows = np.arange(a, b)
    return (full_size[0] - 1 - rows if flip_lat else rows), np.arange(c, d)


def regrid(src, full_size, window=None, subdomain=None, anti_aliasing=False, flip_lat=True):
    """src (Hs, Ws) -> float64 (H_sub, W_sub)"""
    img = np.asarray(src, dtype=np.float64)
    if window is not None:
        img = img[window[0]:window[1], window[2]:window[3]]
    if anti_aliasing:
        img = blur(img, full_size)
    rows, cols = output_indices(full_size, subdomain, flip_lat)
    i0, i1, fy = coordinates(img.shape[0], full_size[0], rows)
    j0, j1, fx = coordinates(img.shape[1], full_size[1], cols)
    fy, fx = fy[:, None], fx[None, :]
    top = (1 - fx) * img[np.ix_(i0, j0)] + fx * img[np.ix_(i0, j1)]
    bot = (1 - fx) * img[np.ix_(i1, j0)] + fx * img[np.ix_(i1, j1)]
    return (1 - fy) * top + fy * bot
