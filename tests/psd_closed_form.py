"""float64 numpy statement of what the reference's ``power_spectral_density`` (py4cast/metrics.py:253-352) computes, shared by
the PSD tests.  Written from the derivation in DESIGN.md ("Power spectrum"), independent of py4cast_amd.ops:

the radial binning indexes the FLATTENED variance spectrum with 2r, 2r-1, 2r+1, so a bin reads row 0 of the orthonormal 2-D
DCT-II only (and, for r = 0, index -1: the last coefficient), and row 0 is the 1-D DCT along W of the plain sum over H."""

import numpy as np
import torch


def bins(H, W):
    """(Rmax, pixels per bin): centre (H//2, W//2) used as (x0, y0), as the reference has it"""
    y, x = np.indices((H, W))
    r = np.sqrt((x - H // 2) ** 2 + (y - W // 2) ** 2).astype(int)
    rmax = min(W - 1, H - 1, int(r.max())) // 2
    return rmax, np.bincount(r[r < rmax], minlength=rmax)[:rmax]


def closed_form(x):
    """x (B, H, W) float64 -> (Rmax,) float64"""
    x = np.asarray(x, dtype=np.float64)
    B, H, W = x.shape
    rmax, count = bins(H, W)
    h, w, k = np.arange(H), np.arange(W), np.arange(2 * rmax)
    s0 = x.sum(axis=1)
    s1 = np.einsum("h,bhw->bw", np.cos(np.pi * (2 * h + 1) * (H - 1) / (2 * H)), x)
    scale = np.where(k == 0, np.sqrt(1.0 / W), np.sqrt(2.0 / W)) / np.sqrt(H)
    X = (s0 @ np.cos(np.pi * np.outer(2 * w + 1, k) / (2 * W))) * scale
    last = np.sqrt(2.0 / H) * np.sqrt(2.0 / W) * (s1 @ np.cos(np.pi * (2 * w + 1) * (W - 1) / (2 * W)))
    sig = (X ** 2).mean(axis=0) / W ** 2
    sig_last = (last ** 2).mean() / W ** 2
    q = np.arange(rmax)
    left = np.where(q == 0, sig_last, sig[np.maximum(2 * q - 1, 0)])
    psd = sig[2 * q] + 0.5 * left + 0.5 * sig[2 * q + 1]
    psd[count == 0] = np.nan
    return psd


def spectra(pred, target, mask, pred_step):
    """(B,T,H,W,F) CPU tensors (mask None = ones) -> (2, F, Rmax) float64: the fp32 products ``tensor * mask`` of the reference,
    then the closed form per feature"""
    out = []
    for t in (pred, target):
        x = t if mask is None else t * mask
        x = x[:, pred_step].double().numpy()
        out.append(np.stack([closed_form(x[..., f]) for f in range(x.shape[-1])]))
    return np.stack(out)


def spectra_torch(pred, target, spec_tensor, pred_step, grid=None):
    """CPU stand-in with the signature of ops.psd's result: float32 tensor"""
    if grid is not None:
        pred, target = pred.unflatten(2, grid), target.unflatten(2, grid)
        spec_tensor = None if spec_tensor is None else spec_tensor.unflatten(2, grid)
    return torch.from_numpy(spectra(pred, target, spec_tensor, pred_step)).float()
