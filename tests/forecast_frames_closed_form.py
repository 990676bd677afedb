"""
What ``ops.forecast_frames`` computes (csrc/forecast_frames.hip), restated on the CPU (test infrastructure, never product code).

``values``:   fp32 torch with the kernel's rounding chain -- ``pred * std`` rounded, ``+ mean`` rounded, ``+ offset`` rounded unless the
              offset is 0 -- the bad mask (not finite, or below the floor) and the colour range of every frame (as given, or min / max
              of the good pixels; (NaN, NaN) without one).  min / max are exact: the kernel's ranges equal these bit for bit.
``indices``:  float64 numpy of the index rule: 255 bad; 0 when vmax == vmin; else x = (v - vmin) / (vmax - vmin), 0 for x < 0, 254 for
              x >= 1, floor(255 x) between; rows flipped (frame row r = grid row H-1-r).  ``band``: the good pixels whose 255 x lies
              within 2^-13 of an integer 1 .. 254, where the kernel's fp32 chain (v - vmin, vmax - vmin, the quotient and the product
              with 255: four roundings of relative 2^-24 on a number below 255, < 2^-14) may fall on the other side.  0 and 255 are no
              such boundaries: x < 0 and floor(255 x) = 0 give the same index, and so do x >= 1 and floor(254.9..).
``compare``:  outside the band equal indices, inside it at most +-1; bad and good never swap anywhere.  -> the band's share.
``CASES``:    the data cases of tests/test_forecast_frames_gpu.py; tests/test_forecast_frames_cpu.py proves the restatement against
              matplotlib on the same ones.
"""
import numpy as np
import torch

BAND = 2.0 ** -13
BAD = 255
INF = float("inf")
NAN = float("nan")


def display_rows(display, features):
    """(K,4) float32 tensor (offset, floor, vmin, vmax) of the drawn features; None -> 0 / -inf / NaN"""
    rows = []
    for f in features:
        off, flo, lo, hi = display[f]
        rows.append((0.0 if off is None else off, -INF if flo is None else flo, NAN if lo is None else lo, NAN if hi is None else hi))
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 4)


def values(pred, std, mean, display, samples=None, features=None):
    """pred (B,T,*S,F) -> v (n,T,K,N) fp32, bad (n,T,K,N) bool, vrange (n,T,K,2) fp32"""
    pred = pred.float().cpu()
    B, T, F = pred.shape[0], pred.shape[1], pred.shape[-1]
    features = list(range(F)) if features is None else list(features)
    samples = list(range(B)) if samples is None else list(samples)
    rows = display_rows(display, features)
    fi = torch.as_tensor(features, dtype=torch.long)
    x = pred.reshape(B, T, -1, F)[torch.as_tensor(samples, dtype=torch.long)].index_select(-1, fi)     # (n,T,N,K)
    a = x * std.float().cpu()[fi]
    v = a + mean.float().cpu()[fi]
    off = rows[:, 0]
    v = torch.where(off != 0, v + off, v)
    v = v.permute(0, 1, 3, 2).contiguous()                                                             # (n,T,K,N)
    flo = rows[:, 1].reshape(1, 1, -1, 1)
    bad = ~torch.isfinite(v) | (v < flo)
    lo = torch.where(bad, torch.full_like(v, INF), v).amin(dim=-1)
    hi = torch.where(bad, torch.full_like(v, -INF), v).amax(dim=-1)
    none = bad.all(dim=-1)
    lo, hi = torch.where(none, torch.full_like(lo, NAN), lo), torch.where(none, torch.full_like(hi, NAN), hi)
    given = ~(torch.isnan(rows[:, 2]) | torch.isnan(rows[:, 3])).reshape(1, 1, -1)
    vrange = torch.stack([torch.where(given, rows[:, 2].reshape(1, 1, -1).expand_as(lo), lo),
                          torch.where(given, rows[:, 3].reshape(1, 1, -1).expand_as(hi), hi)], dim=-1)
    return v, bad, vrange


def indices(v, bad, vrange, H, W):
    """float64 -> dict: index (n,T,K,H,W) uint8, band / bad (n,T,K,H,W) bool, in frame orientation"""
    V = np.asarray(v, dtype=np.float64)
    n, T, K, N = V.shape
    assert N == H * W
    R = np.asarray(vrange, dtype=np.float64)
    vmin, vmax = R[..., 0, None], R[..., 1, None]
    isbad = np.asarray(bad, dtype=bool) | np.isnan(vmin) | np.isnan(vmax)
    flat = vmax == vmin
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = np.where(flat | isbad, 0.0, (np.where(isbad, 0.0, V) - vmin) / (vmax - vmin))
    y = 255.0 * x
    index = np.where(y < 0, 0, np.where(x >= 1.0, 254, np.floor(np.clip(y, 0, 254.5)))).astype(np.int64)
    index = np.where(isbad, BAD, index).astype(np.uint8)
    near = np.rint(y)
    band = (np.abs(y - near) <= BAND) & (near >= 1) & (near <= 254) & ~flat & ~isbad

    def frame(m):
        return np.ascontiguousarray(m.reshape(n, T, K, H, W)[:, :, :, ::-1, :])

    return {"index": frame(index), "band": frame(np.broadcast_to(band, V.shape)), "bad": frame(np.broadcast_to(isbad, V.shape))}


def compare(got, want):
    got = np.asarray(got)
    index, band, bad = want["index"], want["band"], want["bad"]
    assert got.shape == index.shape and got.dtype == np.uint8, (got.shape, got.dtype, index.shape)
    swapped = (got == BAD) != bad
    assert not swapped.any(), f"{int(swapped.sum())} pixels swap bad and good, first at {np.argwhere(swapped)[0].tolist()}"
    diff = np.abs(got.astype(np.int16) - index.astype(np.int16))
    wrong = ~band & (diff != 0)
    assert not wrong.any(), f"{int(wrong.sum())} pixels outside the band differ, first at {np.argwhere(wrong)[0].tolist()}"
    loose = band & (diff > 1)
    assert not loose.any(), f"{int(loose.sum())} pixels inside the band differ by more than 1, first at {np.argwhere(loose)[0].tolist()}"
    return float(band.mean())


def expected(case):
    """(values' triple, indices' dict) of a case"""
    v, bad, vrange = values(case["pred"], case["std"], case["mean"], case["display"], case["samples"], case["features"])
    return (v, bad, vrange), indices(v.numpy(), bad.numpy(), vrange.numpy(), case["H"], case["W"])


# ------------------------------------------------------------------------------------------------ the data cases
# name: (B, T, H, W, F, samples or None, features or None)
SHAPES = {
    "a": (3, 2, 33, 47, 21, (2, 0), None),          # N odd: a byte tail; F off the 16-byte grid
    "b": (2, 2, 16, 20, 5, None, None),
    "c": (2, 2, 20, 52, 60, None, None),            # the benchmark's width
    "d": (2, 2, 12, 36, 64, None, None),            # the bank-conflict width
    "e": (3, 2, 33, 47, 21, (2, 0), (20, 0, 7)),    # the gather form, unsorted
}


def make_case(B, T, H, W, F, samples, features, seed=0):
    """Random data with every special frame and pixel planted.  The first three DRAWN features carry the roles:
      first   std 1, mean 0 (v = pred exactly), range (-3, 5), floor -5: pixels exactly at vmin and vmax, beyond both, exactly at the
              floor and one ulp below it;
      second  the offset feature (std 5, mean 280, offset -273.15), auto-scaled, with +inf and -inf pixels;
      third   auto-scaled: an all-NaN frame, a constant frame, a frame with one good pixel, over the first three drawn frames.
    The other features alternate between a given range and auto-scaling; one has a floor inside its data."""
    g = torch.Generator().manual_seed(1000 + seed)
    N = H * W
    pred = torch.randn(B, T, H, W, F, generator=g)
    std = torch.rand(F, generator=g) * 3 + 0.2
    mean = torch.randn(F, generator=g) * 10
    drawn = list(range(F)) if features is None else list(features)
    smp = list(range(B)) if samples is None else list(samples)
    assert len(drawn) >= 3 and len(smp) * T >= 3
    display = []
    for f in range(F):
        if f % 2:
            display.append((None, None, None, None))
        else:
            lo, hi = float(mean[f] - 2 * std[f]), float(mean[f] + 2 * std[f])
            display.append((None, float(mean[f] - std[f]) if f % 4 == 0 else None, lo, hi))
    flat = pred.reshape(B, T, N, F)
    f0, f1, f2 = drawn[:3]
    std[f0], mean[f0] = 1.0, 0.0
    display[f0] = (None, -5.0, -3.0, 5.0)
    below = float(np.nextafter(np.float32(-5.0), np.float32(-INF)))
    for i, val in enumerate((-3.0, 5.0, 10.0, -4.0, -5.0, below, float(np.nextafter(np.float32(5.0), np.float32(0.0))))):
        flat[smp[0], 0, (7 * i + 3) % N, f0] = val
        flat[smp[-1], T - 1, (5 * i + 1) % N, f0] = val
    std[f1], mean[f1] = 5.0, 280.0
    display[f1] = (-273.15, None, None, None)
    flat[smp[0], 0, 2, f1], flat[smp[0], 0, N - 1, f1], flat[smp[-1], T - 1, N // 2, f1] = INF, -INF, INF
    display[f2] = (None, None, None, None)
    frames = [(s, t) for s in smp for t in range(T)]
    flat[frames[0][0], frames[0][1], :, f2] = NAN
    flat[frames[1][0], frames[1][1], :, f2] = 0.625
    flat[frames[2][0], frames[2][1], :, f2] = NAN
    flat[frames[2][0], frames[2][1], N // 3, f2] = -1.5
    return {"pred": pred, "std": std, "mean": mean, "display": display, "samples": None if samples is None else tuple(samples),
            "features": None if features is None else tuple(features), "H": H, "W": W}


def case(name):
    return make_case(*SHAPES[name], seed=sorted(SHAPES).index(name))


# past one loop trip of every launch (tests/test_forecast_frames_gpu.py asserts that these sizes do it, from the library's own launch
# arithmetic): F, drawn features -- the dense form and the gather form
LOOP_SHAPE = (2, 2, 33, 997)
LOOP_FEATURES = {"dense": (4, (2, 0, 3)), "gather": (8, (5, 0, 3))}


def loop_case(form):
    B, T, H, W = LOOP_SHAPE
    F, features = LOOP_FEATURES[form]
    c = make_case(B, T, H, W, F, None, features, seed=17)
    flat = c["pred"].reshape(B, T, H * W, F)
    flat[1, 1, H * W - 2, features[1]] = 50.0       # the extremes of an auto-scaled frame: in the last, ragged tile and in the first
    flat[1, 1, 1, features[1]] = -50.0
    return c


def all_cases():
    """name -> case, every data case of the GPU test"""
    out = {name: case(name) for name in sorted(SHAPES)}
    out.update({f"loop_{form}": loop_case(form) for form in sorted(LOOP_FEATURES)})
    return out


def synthetic_palette(seed=0):
    """(256,3) uint8 with distinct entries: channel 0 IS the index, so a GIF round trip shows an index off by one"""
    g = np.random.default_rng(seed)
    pal = g.integers(0, 256, size=(256, 3)).astype(np.uint8)
    pal[:, 0] = np.arange(256, dtype=np.uint8)
    return pal
