"""The observers' quantities in float64 numpy, written from the reference's expressions (py4cast/losses.py:143-210,
plots.py:522-542, 606-625): the yardstick of tests/test_observers_cpu.py (against the reference's golden files) and of
tests/test_observers_gpu.py (against ops.eval_sums and the native plotters).  Arrays are (B,T,*S,F); ``mask`` is None, an array of
the same shape, or "nan" (mask = ~isnan(target), target = nan_to_num(target): lightning.py:792-796)."""

import numpy as np


def _np(x):
    if x is None or isinstance(x, (str, np.ndarray)):
        return x
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def resolve(target, mask):
    """(float64 mask, NaN-free float64 target)"""
    target = _np(target).astype(np.float64)
    if isinstance(mask, str):
        assert mask == "nan"
        return (~np.isnan(target)).astype(np.float64), np.nan_to_num(target, nan=0.0)
    if mask is None:
        return np.ones_like(target), target
    return _np(mask).astype(np.float64), target


def diff(pred, target, mask):
    m, t = resolve(target, mask)
    return _np(pred).astype(np.float64) * m - t * m, m      # losses.py:144 / 195


def masked_count(target, mask) -> int:
    """grid points masked for every (b,t,f): losses.py:156 / 197, interior or not"""
    m, _ = resolve(target, mask)
    union = (m != 0).any(axis=(0, 1, m.ndim - 1))
    return int((~union).sum())


def scores(pred, target, mask, interior, std):
    """(2,B,T,F): ScaledLoss on L1Loss, ScaledLoss on MSELoss (losses.py:186-210); interior: (*S) or (*S,1)"""
    d, m = diff(pred, target, mask)
    im = _np(interior).astype(np.float64).reshape(d.shape[2:-1] + (1,))
    spatial = tuple(range(2, d.ndim - 1))
    denom = im.sum() - masked_count(target, mask)
    l1 = (np.abs(d) * im).sum(axis=spatial) / denom
    l2 = np.sqrt((d * d * im).sum(axis=spatial) / denom)
    std = _np(std).astype(np.float64)
    return np.stack([l1 * std, l2 * std])


def loss_map(pred, target, mask, weights, kind):
    """(B,T,*S): WeightedLoss(reduce_spatial_dim=False), losses.py:143-154; kind "MSELoss" / "L1Loss" """
    d, _ = diff(pred, target, mask)
    elem = d * d if kind == "MSELoss" else np.abs(d)
    return (elem * _np(weights).astype(np.float64)).sum(axis=-1)


def weights(state_weight, diff_std, kind):
    """losses.py:119-124"""
    return _np(state_weight).astype(np.float64) / _np(diff_std).astype(np.float64) ** (2.0 if kind == "MSELoss" else 1.0)


def epoch_means(per_update):
    """mean over the concatenated batches (plots.py:541-542, 622-625) of a list of (B, ...) arrays"""
    return np.concatenate(per_update, axis=0).mean(axis=0)
