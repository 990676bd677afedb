"""
What ``ops.map_planes`` / ``ops.map_render`` compute, restated on the CPU (test infrastructure, never product code).

``planes``:  the reference's own fp32 torch expressions (py4cast/plots.py:271, 299-300, 311-312) -- every product and sum rounded on
             its own, so the kernel's output equals it bit for bit.
``render``:  the frame in float64 / numpy, with the masks a comparison needs:
               ``band``      pixels whose 256 x lies within 2^-13 of an integer 1 .. 255, where the fp32 chain of the kernel (three
                             roundings of relative 2^-24, times 256, doubled: <= 2^-14) may fall on the other side;  0 and 256 are
                             no such boundaries (x < 0 and floor(256 x) = 0 give the same index, x >= 1 and floor(255.9..) too);
               ``interior``  pixels with alpha exactly 1: table colour, exact;
               elsewhere (the border, alpha = 0.7 -- no binary fraction) +-1 code value; gaps, NaN values and NaN ranges white.
"""
import numpy as np
import torch

GAP = 8          # ops.MAP_GAP (test_map_frames_cpu.py pins the two to each other)
BAND = 2.0 ** -13


def synthetic_lut(seed=0):
    """(256,3) uint8: distinct neighbours, so an index off by one shows"""
    g = np.random.default_rng(seed)
    lut = g.integers(0, 256, size=(256, 3)).astype(np.uint8)
    lut[:, 0] = np.arange(256, dtype=np.uint8)   # channel 0 IS the index
    return lut


def border_interior(H, W, border=2):
    m = np.zeros((H, W), dtype=np.float32)
    m[border:H - border, border:W - border] = 1.0
    return m


def planes(pred, target, mask, std, mean, features, n, from_nan=False):
    """fp32 torch on the CPU.  pred / target (B,T,*S,F); mask None, a float / bool tensor, or ``from_nan`` (mask = ~isnan(target),
    the NaNs of the target taken as 0).  -> planes (n,T,K,2,N), vrange (n,K,2)"""
    pred, target = pred.float().cpu(), target.float().cpu()
    if from_nan:
        mask = ~torch.isnan(target)
        target = torch.where(mask, target, torch.zeros_like(target))
    p = pred if mask is None else pred * mask.cpu().to(pred.dtype)           # plots.py:271
    idx = torch.as_tensor(list(features), dtype=torch.long)
    std, mean = std.float().cpu(), mean.float().cpu()
    pr = (p * std + mean)[:n].index_select(-1, idx)                           # plots.py:299
    tr = (target * std + mean)[:n].index_select(-1, idx)                      # plots.py:300
    T, K = pred.shape[1], len(idx)
    pr = pr.reshape(n, T, -1, K).permute(0, 1, 3, 2)
    tr = tr.reshape(n, T, -1, K).permute(0, 1, 3, 2)
    out = torch.stack([tr, pr], dim=3).contiguous()                           # (n,T,K,2,N)
    flat = out[:, :, :, 0].permute(0, 2, 1, 3).reshape(n, K, -1)
    vrange = torch.stack([flat.amin(dim=-1), flat.amax(dim=-1)], dim=-1)       # plots.py:311-312 (NaN propagates)
    return out, vrange


def render(planes_, vrange, lut, interior, H, W):
    """float64.  planes_ (n,T,K,2,N), vrange (n,K,2), lut (256,3) uint8, interior (H,W) or (N,) -> dict of frames (n,T,K,H,2W+GAP,3)
    uint8 and boolean masks over the pixels (n,T,K,H,2W+GAP): band, exact (interior and white fills), white"""
    P = np.asarray(planes_, dtype=np.float64)
    R = np.asarray(vrange, dtype=np.float64)
    n, T, K, _, N = P.shape
    assert N == H * W
    a = np.clip(np.asarray(interior, dtype=np.float64).reshape(H, W), 0.7, 1.0)[::-1]        # frame row r = grid row H-1-r
    v = P.reshape(n, T, K, 2, H, W)[:, :, :, :, ::-1, :]
    vmin, vmax = R[:, None, :, 0, None, None, None], R[:, None, :, 1, None, None, None]
    vmin, vmax = np.broadcast_to(vmin, v.shape), np.broadcast_to(vmax, v.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = np.where(vmax == vmin, 0.0, (v - vmin) / (vmax - vmin))
    white = np.isnan(v) | np.isnan(vmin) | np.isnan(vmax) | np.isnan(x)
    y = 256.0 * np.where(white, 0.0, x)
    index = np.where(y < 0, 0, np.where(y >= 256.0, 255, np.floor(np.clip(y, 0, 255.5)))).astype(np.int64)
    near = np.rint(y)
    band = (np.abs(y - near) <= BAND) & (near >= 1) & (near <= 255) & (vmax != vmin) & ~white
    c = np.asarray(lut, dtype=np.float64)[index]                                               # (..., H, W, 3)
    alpha = a[..., None]
    rgb = np.floor(alpha * c + (1.0 - alpha) * 255.0 + 0.5)
    rgb = np.where(white[..., None], 255.0, rgb).astype(np.uint8)
    RW = 2 * W + GAP
    frames = np.full((n, T, K, H, RW, 3), 255, dtype=np.uint8)
    frames[..., :W, :] = rgb[:, :, :, 0]
    frames[..., W + GAP:, :] = rgb[:, :, :, 1]

    def panels(m, fill):
        out = np.full((n, T, K, H, RW), fill, dtype=bool)
        out[..., :W] = m[:, :, :, 0]
        out[..., W + GAP:] = m[:, :, :, 1]
        return out

    is_interior = np.broadcast_to(a == 1.0, white.shape)
    return {"frames": frames, "band": panels(band, False), "white": panels(white, True),
            "exact": panels(is_interior | white, True), "index": index}


def compare(got, want):
    """the comparison the kernel has to pass: outside the band, exact where ``exact``, +-1 elsewhere; -> the band's share"""
    got = np.asarray(got)
    frames, band, exact = want["frames"], want["band"], want["exact"]
    assert got.shape == frames.shape and got.dtype == np.uint8
    keep = ~band
    diff = np.abs(got.astype(np.int16) - frames.astype(np.int16)).max(axis=-1)
    bad = keep & exact & (diff != 0)
    assert not bad.any(), f"{int(bad.sum())} interior / white pixels differ, first at {np.argwhere(bad)[0].tolist()}"
    loose = keep & ~exact & (diff > 1)
    assert not loose.any(), f"{int(loose.sum())} border pixels differ by more than 1, first at {np.argwhere(loose)[0].tolist()}"
    return float(band.mean())
