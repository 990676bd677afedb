"""Writes tests/golden/regrid_*.npz: the regrid chain evaluated with scipy.ndimage, the stated definition of
skimage.transform.resize for the arguments Titan's fit_to_grid passes (py4cast_amd/regrid.py):

    factors = in_shape / out_shape
    if anti_aliasing: img = gaussian_filter(img, sigma=max(0, (factors - 1) / 2), mode="mirror")
    out = zoom(img, 1 / factors, order=1, mode="mirror", grid_mode=True)

followed by the latitude flip and the sub-domain.  Each file holds the parameters of a case and the expected float64 values
on its sub-domain; the source is the analytic field of tests/regrid_closed_form.py (fp32 values), so no source is stored.

    python tests/golden/make_golden_regrid.py
"""
import os
import sys

import numpy as np
from scipy import ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import regrid_closed_form as cf  # noqa: E402

# name: (src_shape, window or None, full_size, subdomain or None, anti_aliasing, flip_lat)
CASES = {
    "up_flip": ((13, 19), None, (37, 53), (5, 30, 7, 49), False, True),
    "up_noflip": ((13, 19), None, (37, 53), (5, 30, 7, 49), False, False),
    "window": ((40, 60), (7, 32, 11, 51), (90, 130), (3, 13, 0, 130), False, True),
    "down_blur": ((45, 70), None, (18, 28), None, True, True),
    "down_noblur": ((45, 70), None, (18, 28), None, False, True),
    "down_blur_strip": ((179, 280), None, (72, 112), (0, 72, 100, 112), True, True),
    "tiny_blur": ((3, 4), None, (1, 2), None, True, True),
    "up_blur_requested": ((7, 9), None, (70, 91), (0, 70, 80, 91), True, True),
    "arpege_to_1s40": ((20, 30), None, (50, 70), (0, 50, 52, 70), True, True),
    "mid_up": ((52, 74), None, (179, 280), (170, 179, 200, 280), False, True),
    "identity": ((25, 42), None, (25, 42), (2, 20, 1, 40), False, True),
    "titan_strip": ((200, 300), (10, 190, 9, 290), (1791, 2801), (1780, 1791, 2700, 2801), False, True),
}


def resize(img, full_size, anti_aliasing):
    factors = np.asarray(img.shape, dtype=np.float64) / np.asarray(full_size, dtype=np.float64)
    if anti_aliasing:
        img = ndi.gaussian_filter(img, sigma=np.maximum(0, (factors - 1) / 2), mode="mirror")
    return ndi.zoom(img, 1 / factors, order=1, mode="mirror", grid_mode=True)


def main():
    for name, (src_shape, window, full_size, sub, aa, flip) in CASES.items():
        img = cf.source_field(src_shape).astype(np.float64)
        if window is not None:
            img = img[window[0]:window[1], window[2]:window[3]]
        full = resize(img, full_size, aa)
        assert full.shape == tuple(full_size), (name, full.shape)
        if flip:
            full = full[::-1]
        a, b, c, d = sub if sub is not None else (0, full_size[0], 0, full_size[1])
        expected = np.ascontiguousarray(full[a:b, c:d])
        np.savez(os.path.join(HERE, f"regrid_{name}.npz"), src_shape=np.array(src_shape), full_size=np.array(full_size),
                 window=np.array(window if window is not None else (0, src_shape[0], 0, src_shape[1])), subdomain=np.array((a, b, c, d)),
                 anti_aliasing=np.array(aa), flip_lat=np.array(flip), expected=expected)
        print(f"regrid_{name}.npz: {expected.shape}, {expected.nbytes} B")


if __name__ == "__main__":
    main()
