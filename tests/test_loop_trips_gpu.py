"""
The streaming kernels of csrc/losses.hip and csrc/rollout.hip against float64 PAST ONE LOOP TRIP.

All of them share one launch shape: a block count capped by the device (loss_blocks / stream_grid / flat_blocks), a grid-stride loop
that takes up what the cap leaves over, a finalize kernel over the per-block partials.  The small-grid tests (test_rollout_gpu.py,
test_flat_step_gpu.py, ...) never enter that loop a second time; the bench-size tests do, but compare the kernel with itself.  Here
every case asserts ``trips >= 2`` for the device it runs on (tests/step_reference.py restates the launch arithmetic;
tests/test_step_reference_cpu.py proves it and proves every case below multi-trip at 256 compute units), calls the kernel once and
compares with the float64 reference (tests/step_reference.py) on the same operands.  Grids are ragged: N is a multiple of neither
the points per wave nor the tile, except where a path demands it.  Buffers the test hands to the library carry 64 grid points
(4 KB for the loss workspace) of 7.0 behind what the call owns, found intact afterwards.

Bars: reductions <= 1e-5 relative; counts, minima, maxima, the mask count exact; element outputs (new state,
next input, build_x, ar_update, unnormalize) bit-equal to the fp32 torch chain; fp32 gradients rtol 1e-5 (with an absolute floor of
4 fp32 ulps of the largest element: the sum loss term + g_next + g_next2 rounds relative to its largest addend); values stored in
bf16 within one bf16 rounding, 2^-8 relative, of the float64 value.
"""
import ctypes

import pytest
import torch

import step_reference as R

pytestmark = pytest.mark.gpu

PAD = 64            # grid points of sentinel behind every buffer the test owns
SENT = 7.0
EPS32 = 2.0 ** -23
BF16_RND = 2.0 ** -8


# ------------------------------------------------------------------------------------------------ the table
# (B, T, F, N, mask mode of the contiguous run, mask mode of the strided run)
LOSS_CASES = [
    (2, 3, 60, 37 * 41, "none", "from_nan"),       # cap 342 blocks; 149 waves take a second trip
    (1, 1, 130, 47 * 53, "u8", "f32"),             # LOSS_MAX_BLOCKS; three feature passes; finalize sums 512 partials
    (1, 2, 256, 47 * 53, "none", "u8"),            # the maximum F: four feature passes, workspace used to its stated size
    (2, 3, 5, 101 * 127, "from_nan", "f32"),       # 8 points per wave; a partial last wave on the second trip
    (4, 4, 1, 191 * 193, "f32", "none"),           # 64 points per wave; cap 128
    (2, 3, 64, 37 * 41, "f32", "from_nan"),        # one full feature pass
    (2, 3, 65, 37 * 41, "u8", "none"),             # one live lane in the second feature pass
]
ACC_V4_CASE = (2, 3, 60, 91 * 97)                  # acc_sums' 16-byte form: 4 points per wave, cap 342 blocks
MASK_COUNT_CASE = (2, 2, 60, 91 * 97)              # 2048-block cap: points 8192.. are second-trip
MOMENTS_CASES = [(3, 47 * 53, 60), (3, 131 * 127, 5)]          # (B, rows, F): LOSS_MAX_BLOCKS at B = 3
# ar_update: (B, N, F, y_cs)
AR_UPDATE_CASES = [(2, 67 * 71, 60, 64), (2, 91 * 97, 21, 64), (2, 191 * 193, 5, 8)]
# build_x: (path, B, T_in, N, F, Fs, Ff, c_pad, mask_on_nan)
BUILD_X_CASES = [
    ("flat", 4, 1, 32780, 60, 4, 5, 96, False),            # 513 tiles over 512 blocks per sample (N % 4 == 0: the path's condition)
    ("flat", 4, 1, 32780, 21, 4, 21, 64, False),
    ("v4", 2, 1, 131 * 127, 60, 4, 5, 96, False),          # odd N: N * Ff % 4 != 0 sends it to the 16-byte kernel
    ("v4", 1, 1, 191 * 193, 21, 4, 21, 64, False),
    ("scalar", 1, 2, 191 * 193, 5, 3, 2, None, True),      # the NaN-mask channel: the scalar kernel
]
UNNORMALIZE_CASE = (2 * 91 * 97, 60)
SUM_GRADS_CASE = (2, 67 * 71, 60)
# the fused step: name -> configuration
_V4 = dict(path="v4", Fs=4, Ff=5)
STEP_CASES = {
    "v4-F60-f32": dict(_V4, B=2, N=91 * 97, F=60, ycs=64, cpad=96, dt="f32", kind="mse", border=True, scaled=True, keep=1.0),
    "v4-F60-bf16": dict(_V4, B=2, N=91 * 97, F=60, ycs=64, cpad=96, dt="bf16", kind="l1", border=False, scaled=True, keep=1.0),
    "v4-F60-nan": dict(_V4, B=2, N=91 * 97, F=60, ycs=64, cpad=96, dt="f32", kind="mse", border=True, scaled=True, keep=1.0, nan=True),
    "v4-F64-f32": dict(_V4, B=2, N=91 * 97, F=64, ycs=64, cpad=96, dt="f32", kind="l1", border=True, scaled=False, keep=1.0),
    "v4-F64-bf16": dict(_V4, B=2, N=91 * 97, F=64, ycs=64, cpad=96, dt="bf16", kind="mse", border=True, scaled=True, keep=0.0),
    "v4-F12": dict(_V4, B=4, N=191 * 193, F=12, ycs=16, cpad=24, dt="f32", kind="mse", border=True, scaled=True, keep=1.0),
    # 64 < F <= 256, F % 4 == 0: the forward runs the scalar kernel, the backward the 16-byte one
    "pair-F128-f32": dict(path="pair", B=2, N=67 * 71, F=128, ycs=128, dt="f32", kind="mse", border=True, scaled=True, keep=1.0),
    "pair-F128-bf16": dict(path="pair", B=2, N=67 * 71, F=128, ycs=128, dt="bf16", kind="l1", border=False, scaled=False, keep=1.0),
    # the flat path: N * F % 4 == 0, last tile 60 points; 512 blocks own 576 tiles
    "flat-F21-f32": dict(path="flat", B=2, N=190 * 194, F=21, ycs=64, Fs=4, Ff=21, cpad=64, dt="f32", kind="mse", border=True, scaled=True,
                         keep=1.0),
    "flat-F21-bf16": dict(path="flat", B=2, N=190 * 194, F=21, ycs=64, Fs=4, Ff=21, cpad=64, dt="bf16", kind="l1", border=True, scaled=False,
                          keep=0.0),
    # NaN masks: the flat path refuses them, F = 21 is off the 16-byte grid
    "scalar-F21-nan": dict(path="scalar", B=2, N=67 * 71, F=21, ycs=64, dt="f32", kind="mse", border=True, scaled=True, keep=1.0, nan=True),
    "scalar-F21-nan-bf16": dict(path="scalar", B=2, N=67 * 71, F=21, ycs=64, dt="bf16", kind="l1", border=False, scaled=True, keep=1.0,
                                nan=True),
}
# the flat kernel with the 1x1 output convolution as its front end (bf16 rows of 64 channels): (F, Fs, Ff, c_pad, kind, border, scaled)
OUT_CONV_CASES = [(60, 4, 5, 96, "mse", True, True), (21, 4, 21, 64, "l1", True, False)]
OUT_CONV_GRID = (2, 190, 194)      # the smallest grid with N * F % 4 == 0 and a 60-point last tile at which 512 blocks own 576 tiles
FORCED_FLAT_CASE = dict(B=2, N=190 * 194, F=60, ycs=64, Fs=4, Ff=5, cpad=96, kind="mse", border=True, scaled=True, keep=1.0)


def _step_trips(cfg):
    """[(trip function, arguments)] of the forward and the backward launch of a fused-step case"""
    B, N, F, ycs = cfg["B"], cfg["N"], cfg["F"], cfg["ycs"]
    return {"v4": [(R.step_v4_trips, (N, F, B)), (R.step_v4_trips, (N, ycs, B))],
            "pair": [(R.step_scalar_trips, (N, F, B)), (R.step_v4_trips, (N, ycs, B))],
            "flat": [(R.step_flat_trips, (N, B))],
            "scalar": [(R.step_scalar_trips, (N, F, B)), (R.step_scalar_trips, (N, ycs, B))]}[cfg["path"]]


def _build_x_trips(path, B, T_in, N, F, Fs, Ff, cpad, nan):
    c = cpad if cpad is not None else T_in * F + Fs + Ff + int(nan)
    return {"flat": (R.build_x_flat_trips, (N, B)), "v4": (R.build_x_v4_trips, (N, c)), "scalar": (R.row_stream_trips, (B * N, c))}[path]


def tabled_trips():
    """(name, trip function, arguments without the CU count) of every launch the cases below are about"""
    for B, T, F, N, _, _ in LOSS_CASES:
        yield f"loss F={F}", R.loss_trips, (N, F, B * T)
    B, T, F, N = ACC_V4_CASE
    yield "acc_sums v4", R.acc_v4_trips, (N, F, B * T)
    B, T, F, N = MASK_COUNT_CASE
    yield "mask count", R.mask_count_trips, (N, F)
    for B, rows, F in MOMENTS_CASES:
        yield f"nan_moments F={F}", R.loss_trips, (rows, F, B)
    for B, N, F, ycs in AR_UPDATE_CASES:
        yield f"ar_update fwd F={F}", R.row_stream_trips, (B * N, F)
        yield f"ar_update bwd F={F}", R.row_stream_trips, (B * N, ycs)
    for case in BUILD_X_CASES:
        yield (f"build_x {case[0]} F={case[4]}",) + _build_x_trips(*case)
    case = BUILD_X_CASES[2]
    yield "build_x_bwd", R.row_stream_trips, (case[1] * case[3], case[2] * case[4])
    yield "unnormalize", R.unnormalize_trips, UNNORMALIZE_CASE
    yield "sum_state_grads", R.sum_state_grads_trips, SUM_GRADS_CASE
    for name, cfg in STEP_CASES.items():
        for fn, args in _step_trips(cfg):
            yield f"step {name}", fn, args
    for case in OUT_CONV_CASES:
        yield f"out_conv F={case[0]}", R.step_flat_trips, (OUT_CONV_GRID[1] * OUT_CONV_GRID[2], OUT_CONV_GRID[0])
    c = FORCED_FLAT_CASE
    yield "step forced flat", R.step_flat_trips, (c["N"], c["B"])
    yield "step forced flat (16-byte side)", R.step_v4_trips, (c["N"], c["F"], c["B"])


# ------------------------------------------------------------------------------------------------ helpers
def _multi_trip(fn, *args):
    from py4cast_amd import _lib as L

    cus = L.lib().p4c_num_cus()
    t = fn(*args, cus)
    assert t >= 2, f"{fn.__name__}{args} makes {t} trip(s) on {cus} compute units: the case has become single-trip"


def _first_trip_points(N, F, nbt):
    """grid points the loss kernels' waves cover on their first trip, on this device"""
    from py4cast_amd import _lib as L

    PP = 64 // R.pow2_ge64(F)
    return 4 * R.loss_blocks(N, PP, nbt, L.lib().p4c_num_cus()) * PP


class Guarded:
    """A buffer of ``shape`` with ``extra`` elements of 7.0 behind it (and the owned part filled with 7.0 too: every element the
    kernel owes is then seen to be written)."""

    def __init__(self, shape, dtype, dev, extra):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.buf = torch.full((n + extra,), SENT, dtype=dtype, device=dev)
        self.t = self.buf[:n].view(*shape)

    def intact(self):
        return bool((self.buf[self.n:] == SENT).all())


def _check_guards(*guards):
    for i, g in enumerate(guards):
        if g is not None:
            assert g.intact(), f"guard {i}: the kernel wrote past the end of its buffer"


def _worst(got, ref, atol=0.0):
    got, ref = got.detach().double(), ref.detach().double()
    err = ((got - ref).abs() - atol).clamp_min(0.0)
    rel = err / ref.abs().clamp_min(1e-300)
    rel = torch.where(err == 0, torch.zeros_like(rel), rel)
    return float(rel.max()) if rel.numel() else 0.0


def _close(what, got, ref, rtol, atol=0.0):
    """|got - ref| <= atol + rtol * |ref| element by element; prints the worst relative excess over atol before asserting"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got.double()).all()), what
    w = _worst(got, ref, atol)
    nrm = float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))
    print(f"[loop-trips] {what}: worst relative error {w:.3e} (bar {rtol:.1e}, floor {atol:.1e}); in the 2-norm {nrm:.3e}")
    assert w <= rtol, (what, w)


def _grad_atol(ref):
    return 4 * EPS32 * float(ref.detach().abs().max())


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _same_bits(what, got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    same = (_bits(got) == _bits(ref)) | (torch.isnan(got) & torch.isnan(ref))
    assert bool(same.all()), f"{what}: {int((~same).sum())} elements differ from the fp32 torch chain"


def _gen(dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (lambda *s: torch.randn(*s, generator=g, device=dev)), (lambda *s: torch.rand(*s, generator=g, device=dev))


def _dt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


# ------------------------------------------------------------------------------------------------ stand-alone losses
def _loss_operands(dev, B, T, F, N, mode, strided, seed):
    """pred = target + 0.3 noise (the cross term of acc_sums is then well conditioned); strided: prediction and target are the
    slices [:, 1:1+T] of (B, T+2, N, F) buffers; masked points (all of b, t, f) sit on second-trip indices."""
    rn, ru = _gen(dev, seed)
    Tb = T + 2 if strided else T
    tbuf, nbuf = rn(B, Tb, N, F), rn(B, Tb, N, F)
    pbuf = tbuf + 0.3 * nbuf
    sl = slice(1, 1 + T) if strided else slice(0, T)
    dead = torch.tensor([N - 2, N - 3, N - 37, 5], device=dev)
    mask = None
    if mode == "from_nan":
        tbuf[:, :, dead] = float("nan")
        tbuf[0, sl.start, 11, 0] = float("nan")
        tbuf[B - 1, sl.stop - 1, N - 5, F - 1] = float("nan")
    elif mode in ("f32", "u8"):
        keep = ru(B, T, N, F) > 0.1
        keep[:, :, dead] = False
        mask = torch.where(keep, torch.where(ru(B, T, N, F) > 0.5, 1.0, 0.5), 0.0) if mode == "f32" else keep.to(torch.uint8)
    pred, target = pbuf[:, sl], tbuf[:, sl]
    interior = (ru(N) > 0.2).float()
    # the points on either side of the trip boundary and the last one count in the reduced losses: one dropped or doubled point there
    # cannot hide behind a zero of the interior mask
    first = _first_trip_points(N, F, B * T)
    interior[[first - 1, first, first + 1, N - 1]] = 1.0
    return dict(pred=pred, target=target, mask=mask, interior=interior, weights=ru(F) + 0.5, std=ru(F) + 0.5, clim=rn(F) * 0.1,
                gout=ru(B, T) + 0.5, num_interior=float(interior.sum()))


def _loss_references(c, kind, mode):
    p = c["pred"].double().requires_grad_(True)
    w = R.weighted_loss(p, c["target"], c["weights"], c["interior"], kind, mode, c["mask"])
    (dpred,) = torch.autograd.grad((w * c["gout"].double()).sum(), p)
    return dict(w=w.detach(), dpred=dpred, map=R.weighted_loss_map(c["pred"], c["target"], c["weights"], kind, mode, c["mask"]),
                s=R.scaled_loss(c["pred"], c["target"], c["std"], c["interior"], kind, mode, c["mask"]),
                acc=R.acc_sums(c["pred"], c["target"], c["clim"], mode, c["mask"]), count=R.masked_count(c["target"], mode, c["mask"]))


def _check_losses(tag, got, ref):
    _close(f"{tag} weighted_loss", got["w"], ref["w"], 1e-5)
    _close(f"{tag} weighted_loss_map", got["map"], ref["map"], 1e-5)
    _close(f"{tag} scaled_loss", got["s"], ref["s"], 1e-5)
    _close(f"{tag} acc_sums", got["acc"], ref["acc"], 1e-5)
    _close(f"{tag} dpred", got["dpred"], ref["dpred"], 1e-5, _grad_atol(ref["dpred"]) * 0.25)   # (one product chain: 1 ulp floor)


def _spec(ops, L, mode, mask):
    code = {"none": L.MASK_NONE, "from_nan": L.MASK_FROM_NAN, "f32": L.MASK_F32, "u8": L.MASK_U8}[mode]
    return ops.MaskSpec(code, mask)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B,T,F,N,mode,_m2", LOSS_CASES, ids=[f"F{c[2]}" for c in LOSS_CASES])
def test_losses_contiguous(gpu_device, kind, B, T, F, N, mode, _m2):
    """Through the ops wrappers (which own outputs and workspace): forward, map, backward by autograd, scaled loss, acc_sums."""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    _multi_trip(R.loss_trips, N, F, B * T)
    c = _loss_operands(gpu_device, B, T, F, N, mode, False, 100 + F)
    ref = _loss_references(c, kind, mode)
    spec, code = _spec(ops, L, mode, c["mask"]), ops.loss_kind_code(kind)
    count = ops.masked_count(spec, c["target"])
    assert (0 if count is None else int(count)) == ref["count"]
    p = c["pred"].clone().requires_grad_(True)
    w = ops.weighted_loss(p, c["target"], spec, c["weights"], c["interior"], c["num_interior"], code, count=count)
    (w * c["gout"]).sum().backward()
    got = dict(w=w.detach(), dpred=p.grad, map=ops.weighted_loss_map(c["pred"], c["target"], spec, c["weights"], code),
               s=ops.scaled_loss(c["pred"], c["target"], spec, c["std"], c["interior"], c["num_interior"], code, count=count),
               acc=ops.acc_sums(c["pred"], c["target"], spec, c["clim"]))
    _check_losses(f"F={F} {kind} {mode}", got, ref)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B,T,F,N,_m1,mode", LOSS_CASES, ids=[f"F{c[2]}" for c in LOSS_CASES])
def test_losses_strided(gpu_device, kind, B, T, F, N, _m1, mode):
    """Through the C ABI with strided leading dimensions -- prediction and target are slices [:, 1:1+T] of (B, T+2, N, F) buffers --
    and guarded outputs, gradient and workspace."""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    _multi_trip(R.loss_trips, N, F, B * T)
    dev = gpu_device
    c = _loss_operands(dev, B, T, F, N, mode, True, 200 + F)
    ref = _loss_references(c, kind, mode)
    spec, code = _spec(ops, L, mode, c["mask"]), ops.loss_kind_code(kind)
    pred, target = c["pred"], c["target"]
    assert pred.stride(0) == (T + 2) * N * F and pred.data_ptr() != pred._base.data_ptr() and pred[0, 0].is_contiguous()
    pbs, pts, gbs, gts = pred.stride(0), pred.stride(1), target.stride(0), target.stride(1)
    count = ops.masked_count(spec, target)
    assert (0 if count is None else int(count)) == ref["count"]
    ws_floats = L.lib().p4c_loss_workspace_bytes(B, T, N, F) // 4
    ws, ws3 = Guarded((ws_floats,), torch.float32, dev, 1024), Guarded((3 * ws_floats,), torch.float32, dev, 1024)
    out, omap = Guarded((B, T), torch.float32, dev, PAD), Guarded((B, T, N), torch.float32, dev, PAD)
    dpred, outs = Guarded((B, T, N, F), torch.float32, dev, PAD * F), Guarded((B, T, F), torch.float32, dev, PAD * F)
    acc = Guarded((3, B, T, F), torch.float32, dev, PAD * F)
    st, ni = L.stream(dev), c["num_interior"]
    head = (L.ptr(pred), pbs, pts, L.ptr(target), gbs, gts, L.ptr(spec.tensor), spec.mode)
    L.call("p4c_weighted_loss_fwd", *head, L.ptr(c["weights"]), L.ptr(c["interior"]), ni, L.ptr(count), code, L.ptr(out.t), L.ptr(ws.t),
           B, T, N, F, st)
    L.call("p4c_weighted_loss_map", *head, L.ptr(c["weights"]), code, L.ptr(omap.t), B, T, N, F, st)
    L.call("p4c_weighted_loss_bwd", L.ptr(c["gout"]), *head, L.ptr(c["weights"]), L.ptr(c["interior"]), ni, L.ptr(count), code,
           L.ptr(dpred.t), T * N * F, N * F, B, T, N, F, st)
    torch.cuda.synchronize()
    _check_guards(ws, out, omap, dpred)
    L.call("p4c_scaled_loss_fwd", *head, L.ptr(c["std"]), L.ptr(c["interior"]), ni, L.ptr(count), code, L.ptr(outs.t), L.ptr(ws.t),
           B, T, N, F, st)
    L.call("p4c_acc_sums", *head, L.ptr(c["clim"]), L.ptr(acc.t), L.ptr(ws3.t), B, T, N, F, st)
    torch.cuda.synchronize()
    _check_guards(ws, ws3, outs, acc)
    _check_losses(f"F={F} {kind} {mode} strided", dict(w=out.t, map=omap.t, dpred=dpred.t, s=outs.t, acc=acc.t), ref)


@pytest.mark.parametrize("mode", ["none", "from_nan"])
def test_acc_sums_16_byte_form(gpu_device, mode):
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    B, T, F, N = ACC_V4_CASE
    _multi_trip(R.acc_v4_trips, N, F, B * T)
    c = _loss_operands(gpu_device, B, T, F, N, mode, False, 300)
    got = ops.acc_sums(c["pred"], c["target"], _spec(ops, L, mode, None), c["clim"])
    _close(f"acc_sums v4 {mode}", got, R.acc_sums(c["pred"], c["target"], c["clim"], mode), 1e-5)


@pytest.mark.parametrize("mode", ["from_nan", "u8"])
def test_mask_all_zero_count(gpu_device, mode):
    """The all-masked points sit on second-trip indices (8192.. with the 2048-block cap), N - 1 among them; exact."""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    B, T, F, N = MASK_COUNT_CASE
    _multi_trip(R.mask_count_trips, N, F)
    dev = gpu_device
    rn, ru = _gen(dev, 310)
    first_trip = 4 * R.mask_count_blocks(N, F, L.lib().p4c_num_cus()) * (64 // R.pow2_ge64(F))
    dead = torch.tensor([N - 1, N - 2, first_trip, first_trip + 1, (first_trip + N) // 2], device=dev)
    assert int(dead.min()) >= first_trip
    target = rn(B, T, N, F)
    if mode == "from_nan":
        target[:, :, dead] = float("nan")
        target[0, 1, 17] = float("nan")                  # masked in one (b, t) only: not counted
        target[:, :, 18, : F - 1] = float("nan")         # one live feature: not counted
        spec = ops.MaskSpec(L.MASK_FROM_NAN)
        want = R.masked_count(target, "from_nan")
    else:
        m = (ru(B, T, N, F) > 0.3).to(torch.uint8)
        m[:, :, dead] = 0
        m[:, :, 19] = 0
        m[B - 1, T - 1, 19, F - 1] = 1                   # one set byte in the last (b, t, f): not counted
        spec = ops.MaskSpec(L.MASK_U8, m)
        want = R.masked_count(target, "u8", m)
    assert want == dead.numel()
    assert int(ops.masked_count(spec, target)) == want


@pytest.mark.parametrize("diff", [False, True], ids=["x", "x_next-x"])
@pytest.mark.parametrize("B,rows,F", MOMENTS_CASES, ids=[f"F{c[2]}" for c in MOMENTS_CASES])
def test_nan_moments(gpu_device, B, rows, F, diff):
    """sums, squares, count, min, max per (sample, feature): means and variances <= 1e-5, the rest exact.  The data are offset from
    zero (mean 1.5, spread 1), so that mean and variance are well conditioned."""
    from py4cast_amd import _lib as L
    from py4cast_amd import dataset_stats as ds

    _multi_trip(R.loss_trips, rows, F, B)
    dev = gpu_device
    rn, ru = _gen(dev, 320 + F)
    x = rn(B, rows, F) + 1.5
    x[0, rows - 1, 0] = float("nan")
    x[B - 1, rows // 2:, F - 1] = float("nan")
    xn = x + 0.5 * rn(B, rows, F) + 0.7 if diff else None
    ref = R.nan_moments(x, xn)
    if not diff:
        got = ds.nan_moments(x)
    else:
        out = Guarded((5, B, F), torch.float32, dev, PAD * F)
        ws = Guarded((5 * L.lib().p4c_loss_workspace_bytes(B, 1, rows, F) // 4,), torch.float32, dev, 1024)
        L.call("p4c_nan_moments", L.ptr(x), L.ptr(xn), x.stride(0), L.ptr(out.t), L.ptr(ws.t), B, rows, F, L.stream(dev))
        torch.cuda.synchronize()
        _check_guards(out, ws)
        got = out.t
    assert torch.equal(got[2].double(), ref[2]), "count"
    assert torch.equal(got[3].double(), ref[3]) and torch.equal(got[4].double(), ref[4]), "min / max"
    cnt = ref[2]
    mean, mean_ref = got[0].double() / cnt, ref[0] / cnt
    _close("nan_moments mean", mean, mean_ref, 1e-5)
    _close("nan_moments variance", got[1].double() / cnt - mean ** 2, ref[1] / cnt - mean_ref ** 2, 1e-5)


# ------------------------------------------------------------------------------------------------ element kernels
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,N,F,ycs", AR_UPDATE_CASES, ids=[f"F{c[2]}" for c in AR_UPDATE_CASES])
def test_ar_update(gpu_device, B, N, F, ycs, dt):
    from py4cast_amd import ops

    _multi_trip(R.row_stream_trips, B * N, F)
    _multi_trip(R.row_stream_trips, B * N, ycs)
    dev = gpu_device
    rn, ru = _gen(dev, 400 + F)
    scaled, nan = F != 21, F == 60
    prev, y, bs = rn(B, N, F), rn(B, N, ycs).to(_dt(dt)), rn(B, N, F)
    if nan:
        prev[0, N - 1, 3] = float("nan")
        bs[1, N - 2] = float("nan")
    std, mean = (ru(F) + 0.5, rn(F) * 0.01) if scaled else (None, None)
    interior = (ru(N) > 0.2).float()
    bm = 1.0 - interior
    pl, yl = prev.clone().requires_grad_(True), y.clone().requires_grad_(True)
    got = ops.ar_update(pl, yl, bs if scaled else None, std, mean, bm if scaled else None, interior if scaled else None, 1.0, nan)
    args = (bs if scaled else None, std, mean, bm if scaled else None, interior if scaled else None, 1.0, nan)
    _same_bits("ar_update", got.detach(), R.ar_update(prev, y, *args, dtype=torch.float32))
    g = rn(B, N, F)
    got.backward(g)
    p64, y64 = prev.double().requires_grad_(True), y.double().requires_grad_(True)
    (R.ar_update(p64, y64, *args) * g.double()).sum().backward()
    ok = ~torch.isnan(prev)      # (where prev holds a NaN the kernel passes the gradient through nan_to_num, autograd stops it)
    _close("ar_update dprev", pl.grad[ok], p64.grad[ok], 1e-5)
    if dt == "bf16":
        _close("ar_update dy (bf16)", yl.grad, y64.grad, BF16_RND)
    else:
        _close("ar_update dy", yl.grad, y64.grad, 1e-5)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("path,B,T_in,N,F,Fs,Ff,cpad,nan", BUILD_X_CASES, ids=[f"{c[0]}-F{c[4]}" for c in BUILD_X_CASES])
def test_build_x(gpu_device, path, B, T_in, N, F, Fs, Ff, cpad, nan, dt):
    from py4cast_amd import ops

    fn, args = _build_x_trips(path, B, T_in, N, F, Fs, Ff, cpad, nan)
    _multi_trip(fn, *args)
    dev = gpu_device
    rn, ru = _gen(dev, 500 + F)
    prev, st, fo = rn(B, T_in, N, F), ru(B, N, Fs), ru(B, N, Ff) * 100
    if nan:
        prev[0, 0, N - 1, 1] = float("nan")
        fo[B - 1, N - 3, 0] = float("nan")
        prev[0, T_in - 1, 9000] = float("nan")
    if path == "flat":
        assert (N * F) % 4 == 0 and (N * Fs) % 4 == 0 and (N * Ff) % 4 == 0
    if path == "v4":
        assert (N * Ff) % 4 != 0 or (N * F) % 4 != 0
    pl = prev.clone().requires_grad_(True)
    got = ops.build_x(pl, st, fo, nan, c_pad=cpad, dtype=_dt(dt))
    _same_bits("build_x", got.detach(), R.build_x(prev, st, fo, cpad, _dt(dt), nan))
    if path == "v4" and F == 60:
        _multi_trip(R.row_stream_trips, B * N, T_in * F)
        g = rn(*got.shape).to(_dt(dt))
        got.backward(g)
        want = torch.stack([g[..., t * F:(t + 1) * F].float() for t in range(T_in)], dim=1)
        _same_bits("build_x_bwd", pl.grad, want)


def test_unnormalize(gpu_device):
    from py4cast_amd import ops

    rows, F = UNNORMALIZE_CASE
    _multi_trip(R.unnormalize_trips, rows, F)
    rn, ru = _gen(gpu_device, 600)
    x, std, mean = rn(rows, F), ru(F) + 0.5, rn(F)
    out = Guarded((rows, F), torch.float32, gpu_device, PAD * F)
    ops.unnormalize(x, std, mean, out=out.t)
    torch.cuda.synchronize()
    _check_guards(out)
    _same_bits("unnormalize", out.t, R.unnormalize(x, std, mean, dtype=torch.float32))


def test_sum_state_grads(gpu_device):
    """out = fp32 rows + fp32 strided rows + a channel block of bf16 rows, in that order: bit-equal to the fp32 torch chain."""
    from py4cast_amd import _lib as L

    B, N, F = SUM_GRADS_CASE
    _multi_trip(R.sum_state_grads_trips, B, N, F)
    dev = gpu_device
    rn, _ = _gen(dev, 610)
    a, bbuf, c = rn(B, N, F), rn(B, 3, N, F), rn(B, N, 128).bfloat16()
    b = bbuf[:, 1]
    srcs = (ctypes.c_void_p * 8)()
    sbs, scs, soff, sdt = (ctypes.c_int64 * 8)(), (ctypes.c_int * 8)(), (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
    for k, (t, bs, cs, off, code) in enumerate([(a, N * F, F, 0, L.F32), (b, bbuf.stride(0), F, 0, L.F32), (c, N * 128, 128, F, L.BF16)]):
        srcs[k], sbs[k], scs[k], soff[k], sdt[k] = t.data_ptr(), bs, cs, off, code
    out = Guarded((B, N, F), torch.float32, dev, PAD * F)
    L.call("p4c_sum_state_grads", L.ptr(out.t), N * F, 3, srcs, sbs, scs, soff, sdt, B, N, F, L.stream(dev))
    torch.cuda.synchronize()
    _check_guards(out)
    _same_bits("sum_state_grads", out.t, (a + b) + c[..., F:2 * F].float())


# ------------------------------------------------------------------------------------------------ the fused AR step
def _step_operands(dev, cfg, seed):
    B, N, F, ycs, dt = cfg["B"], cfg["N"], cfg["F"], cfg["ycs"], _dt(cfg["dt"])
    Fs, Ff = cfg.get("Fs", 0), cfg.get("Ff", 0)
    rn, ru = _gen(dev, seed)
    c = dict(y=rn(B, N, ycs).to(dt), prev=rn(B, N, F), tgt=rn(B, N, F), weights=ru(F) + 0.5, gloss=ru(B) + 0.5, g1=rn(B, N, F),
             g2=rn(B, N, ycs).to(dt), interior=(ru(N) > 0.2).float(), statics=ru(B, N, max(Fs, 1)), forcing=ru(B, N, max(Ff, 1)) * 100)
    c["border"] = (1.0 - c["interior"]) if cfg["border"] else None
    c["std"], c["mean"] = (ru(F) + 0.5, rn(F) * 0.01) if cfg["scaled"] else (None, None)
    c["count"] = None
    if cfg.get("nan"):
        c["tgt"][:, N - 1] = float("nan")                # masked for every (b, f): counted
        c["tgt"][:, N - 70] = float("nan")
        c["tgt"][0, N - 2, F - 1] = float("nan")
        c["prev"][B - 1, N - 3, 0] = float("nan")
        c["count"] = torch.tensor([R.masked_count(c["tgt"].unsqueeze(1), "from_nan")], dtype=torch.int32, device=dev)
        assert int(c["count"]) == 2
    return c


def _step_forward(L, c, cfg, variant):
    """variant: plain | next | saved (next input + saved loss gradients) | free | free_next.  Returns the guarded outputs."""
    B, N, F, ycs, dt = cfg["B"], cfg["N"], cfg["F"], cfg["ycs"], _dt(cfg["dt"])
    Fs, Ff, cpad = cfg.get("Fs", 0), cfg.get("Ff", 0), cfg.get("cpad", 0)
    dev = c["y"].device
    code = L.dtype_code(dt)
    mode = L.MASK_FROM_NAN if cfg.get("nan") else L.MASK_NONE
    kind = R.KINDS.index(cfg["kind"])
    ns, loss = Guarded((B, N, F), torch.float32, dev, PAD * F), Guarded((B,), torch.float32, dev, PAD)
    ws = Guarded((L.lib().p4c_loss_workspace_bytes(B, 1, N, 1) // 4,), torch.float32, dev, 1024)
    xn = Guarded((B, N, cpad), dt, dev, PAD * cpad) if variant in ("next", "saved", "free_next") else None
    lgr = Guarded((B, N, F), torch.bfloat16, dev, PAD * F) if variant == "saved" else None
    st = L.stream(dev)
    free = variant in ("free", "free_next")
    tgt = c["tgt"] if (cfg["border"] or not free) else None        # a free step that forces nothing has no target
    state = [L.ptr(c["prev"]), N * F, L.ptr(c["y"]), code, ycs, L.ptr(tgt), N * F, L.ptr(c["std"]), L.ptr(c["mean"]), L.ptr(c["border"]),
             L.ptr(c["interior"]), L.ptr(ns.t), N * F]
    nxt = [L.ptr(xn.t) if xn else None, cpad, L.ptr(c["statics"]), N * max(Fs, 1), Fs, L.ptr(c["forcing"]), N * max(Ff, 1), Ff]
    if free:
        L.call("p4c_ar_update_next", *state, int(bool(cfg.get("nan"))), B, N, F, cfg["keep"], *nxt, st)
    else:
        args = state + [L.ptr(c["weights"]), float(c["interior"].sum()), L.ptr(c["count"]), kind, mode, L.ptr(loss.t), 1, L.ptr(ws.t), B, N, F,
                        cfg["keep"]]
        if variant == "plain":
            L.call("p4c_ar_update_loss_fwd", *args, st)
        elif variant == "next":
            L.call("p4c_ar_update_loss_fwd_next", *args, *nxt, st)
        else:
            L.call("p4c_ar_update_loss_fwd_next_saved", *args, *nxt, L.ptr(lgr.t), N * F, st)
    torch.cuda.synchronize()
    _check_guards(ns, loss, ws, xn, lgr)
    return ns, loss, xn, lgr


def _step_backward(L, c, cfg, variant, ns=None, lgr=None, first=False, last=False):
    """variant: plain (recomputes the loss gradient from new state and target) | saved | free.  first: no dprev; last: no upstream."""
    B, N, F, ycs, dt = cfg["B"], cfg["N"], cfg["F"], cfg["ycs"], _dt(cfg["dt"])
    dev = c["y"].device
    code = L.dtype_code(dt)
    mode = L.MASK_FROM_NAN if cfg.get("nan") else L.MASK_NONE
    kind = R.KINDS.index(cfg["kind"])
    dy = Guarded((B, N, ycs), dt, dev, PAD * ycs)
    dprev = None if first else Guarded((B, N, F), torch.float32, dev, PAD * F)
    g1, g2 = (None, None) if last else (c["g1"], c["g2"])
    ni, st = float(c["interior"].sum()), L.stream(dev)
    up = [L.ptr(g1), N * F, L.ptr(g2), code, ycs]
    tail = [L.ptr(dy.t), code, ycs, L.ptr(dprev.t) if dprev else None, N * F, B, N, F, cfg["keep"], st]
    force = int(bool(cfg["border"]))
    if variant == "free":
        L.call("p4c_ar_update_next_bwd", *up, L.ptr(c["std"]), L.ptr(c["interior"]), force, *tail)
    elif variant == "saved":
        L.call("p4c_ar_update_loss_bwd_saved", *up, L.ptr(c["gloss"]), 1, L.ptr(lgr), N * F, L.ptr(c["std"]), L.ptr(c["interior"]), force,
               L.ptr(c["weights"]), ni, L.ptr(c["count"]), kind, mode, *tail)
    else:
        L.call("p4c_ar_update_loss_bwd", *up, L.ptr(c["gloss"]), 1, L.ptr(ns), N * F, L.ptr(c["tgt"]), N * F, L.ptr(c["std"]),
               L.ptr(c["interior"]), force, L.ptr(c["weights"]), ni, L.ptr(c["count"]), kind, mode, *tail)
    torch.cuda.synchronize()
    _check_guards(dy, dprev)
    return dy, dprev


def _step_reference(c, cfg, state, loss=True, with_next=False):
    """float64 reference at the kernel's stored state + the float64 leaves for fused_step_grads"""
    y64, p64 = c["y"].double().requires_grad_(True), c["prev"].double().requires_grad_(True)
    nxt = (c["statics"][..., : cfg.get("Fs", 0)], c["forcing"][..., : cfg.get("Ff", 0)], cfg["cpad"], _dt(cfg["dt"])) if with_next else None
    forced = cfg["border"]
    out = R.fused_step(p64, y64, c["tgt"] if (loss or forced) else None, c["std"], c["mean"], c["border"],
                       c["interior"] if (loss or forced) else None, c["weights"] if loss else None, cfg["kind"], cfg["keep"],
                       bool(cfg.get("nan")), loss=loss, next_input=nxt, state=state)
    return out, y64, p64


def _check_state(tag, c, cfg, ns, free=False):
    forced = cfg["border"]
    chain = R.fused_step(c["prev"], c["y"], c["tgt"] if forced or not free else None, c["std"], c["mean"], c["border"],
                         c["interior"] if forced or not free else None, None, cfg["kind"], cfg["keep"], bool(cfg.get("nan")), loss=False,
                         dtype=torch.float32)["new_state"]
    _same_bits(f"{tag} new state", ns.t, chain)


def _check_grads(tag, c, cfg, dy, dprev, dy_ref, dprev_ref):
    """(dprev where the previous state holds a NaN is left out: the kernels pass the gradient through nan_to_num, autograd stops it)"""
    F = cfg["F"]
    if cfg["dt"] == "bf16":
        _close(f"{tag} dy (bf16)", dy.t, dy_ref, BF16_RND, _grad_atol(dy_ref))
    else:
        _close(f"{tag} dy", dy.t, dy_ref, 1e-5, _grad_atol(dy_ref))
    assert float(dy.t[..., F:].float().abs().max() if cfg["ycs"] > F else 0.0) == 0.0, "channels >= F of dy"
    if dprev is not None:
        ok = ~torch.isnan(c["prev"])
        _close(f"{tag} dprev", dprev.t[ok], dprev_ref[ok], 1e-5, _grad_atol(dprev_ref))


def _run_step_case(L, name, cfg, dev):
    """Every entry point the case's path serves, each once, each against the reference."""
    c = _step_operands(dev, cfg, 700 + sum(map(ord, name)))
    has_next = cfg["path"] in ("v4", "flat") and not cfg.get("nan")     # (the NaN-mask input channel is built by p4c_build_x)
    # ---- the loss-carrying step: forward (+ next input, + saved loss gradients), both backward forms
    fwd_variants = ["plain"] + (["next", "saved"] if has_next else [])
    for variant in fwd_variants:
        ns, loss, xn, lgr = _step_forward(L, c, cfg, variant)
        tag = f"{name} {variant}"
        _check_state(tag, c, cfg, ns)
        out, y64, p64 = _step_reference(c, cfg, ns.t, with_next=xn is not None)
        _close(f"{tag} loss", loss.t, out["loss"].detach(), 1e-5)
        if xn is not None:
            _same_bits(f"{tag} next input", xn.t, out["x_next"])
        if lgr is not None:
            _close(f"{tag} saved loss gradient (bf16)", lgr.t, out["lgrad"], BF16_RND)
        if variant == "plain":
            dy, dprev = _step_backward(L, c, cfg, "plain", ns=ns.t)
            dy_ref, dprev_ref = R.fused_step_grads(out, y64, p64, c["gloss"], c["g1"], c["g2"])
            _check_grads(f"{tag} bwd", c, cfg, dy, dprev, dy_ref, dprev_ref)
        if variant == "saved":
            dy, dprev = _step_backward(L, c, cfg, "saved", lgr=lgr.t)
            dy_ref, dprev_ref = R.fused_step_grads(out, y64, p64, c["gloss"], c["g1"], c["g2"], interior_mask=c["interior"],
                                                   weights=c["weights"], lgrad=lgr.t)
            _check_grads(f"{tag} bwd_saved", c, cfg, dy, dprev, dy_ref, dprev_ref)
    # the first / last AR step's backward: no dprev, no upstream gradient
    out, y64, p64 = _step_reference(c, cfg, ns.t)
    dy, _ = _step_backward(L, c, cfg, "plain", ns=ns.t, first=True, last=True)
    dy_ref, _ = R.fused_step_grads(out, y64, p64, c["gloss"])
    _check_grads(f"{name} bwd (first, last)", c, cfg, dy, None, dy_ref, None)
    # ---- the free step and its adjoint
    variant = "free_next" if has_next else "free"
    ns, _, xn, _ = _step_forward(L, c, cfg, variant)
    _check_state(f"{name} free", c, cfg, ns, free=True)
    out, y64, p64 = _step_reference(c, cfg, ns.t, loss=False, with_next=xn is not None)
    if xn is not None:
        _same_bits(f"{name} free next input", xn.t, out["x_next"])
    dy, dprev = _step_backward(L, c, cfg, "free")
    dy_ref, dprev_ref = R.fused_step_grads(out, y64, p64, None, c["g1"], c["g2"])
    _check_grads(f"{name} free bwd", c, cfg, dy, dprev, dy_ref, dprev_ref)


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_fused_step(gpu_device, name):
    from py4cast_amd import _lib as L

    cfg = STEP_CASES[name]
    for fn, args in _step_trips(cfg):
        _multi_trip(fn, *args)
    if cfg["path"] == "flat":
        assert (cfg["N"] * cfg["F"]) % 4 == 0 and cfg["N"] % 64 == 60
    _run_step_case(L, name, cfg, gpu_device)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_fused_step_flat_and_16_byte_kernels_on_the_same_operands(gpu_device, diag_library, monkeypatch, dt):
    """F = 60 at the flat case's grid: P4C_FORCE_FLAT_STEP=1 puts the flat kernels where the 16-byte ones serve by default; both
    against the reference on the same multi-trip operands."""
    from py4cast_amd import _lib as L

    cfg = dict(FORCED_FLAT_CASE, dt=dt)
    _multi_trip(R.step_flat_trips, cfg["N"], cfg["B"])
    _multi_trip(R.step_v4_trips, cfg["N"], cfg["F"], cfg["B"])
    for force in ("0", "1"):
        monkeypatch.setenv("P4C_FORCE_FLAT_STEP", force)
        _run_step_case(L, f"forced-flat={force} {dt}", dict(cfg, path="flat" if force == "1" else "v4"), gpu_device)


@pytest.mark.parametrize("F,Fs,Ff,cpad,kind,border,scaled", OUT_CONV_CASES, ids=[f"F{c[0]}" for c in OUT_CONV_CASES])
def test_out_conv_front_end(gpu_device, F, Fs, Ff, cpad, kind, border, scaled):
    """p4c_out_conv_update_loss_fwd / _update_fwd: the flat kernel forms y = conv1x1(relu(a * scale + shift)) on the matrix cores at the
    head of every tile.  The operand y of the reference is the 1x1 convolution's own launch on the same a (the rows the two-kernel route
    stores: tests/test_fused_tail_gpu.py holds the two equal on one trip); everything downstream of y is held to the reference."""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops_model as om

    B, H, W = OUT_CONV_GRID
    N = H * W
    cfg = dict(path="flat", B=B, N=N, F=F, ycs=64, Fs=Fs, Ff=Ff, cpad=cpad, dt="bf16", kind=kind, border=border, scaled=scaled, keep=1.0)
    _multi_trip(R.step_flat_trips, N, B)
    assert (N * F) % 4 == 0 and N % 64 == 60
    dev = gpu_device
    c = _step_operands(dev, cfg, 900 + F)
    rn, ru = _gen(dev, 910 + F)
    a, sc, sh, w = rn(B, H, W, 64).bfloat16(), ru(B, 64) + 0.5, rn(B, 64) * 0.3, rn(F, 64, 1, 1) * 0.2
    c["y"] = om.conv_fwd(a, om.prep_weights(w, False, 64, 64, compute="bf16"), 1, in_scale=sc, in_shift=sh, in_relu=True,
                         compute="bf16").reshape(B, N, 64)
    wflat = w.reshape(F, 64).contiguous()
    st, kcode = L.stream(dev), R.KINDS.index(kind)
    front = [L.ptr(a), L.ptr(sc), L.ptr(sh), L.ptr(wflat), F]
    nxt = [cpad, L.ptr(c["statics"]), N * Fs, Fs, L.ptr(c["forcing"]), N * Ff, Ff]
    for loss in (True, False):
        ns, lossv = Guarded((B, N, F), torch.float32, dev, PAD * F), Guarded((B,), torch.float32, dev, PAD)
        ws = Guarded((L.lib().p4c_loss_workspace_bytes(B, 1, N, 1) // 4,), torch.float32, dev, 1024)
        xn, lgr = Guarded((B, N, cpad), torch.bfloat16, dev, PAD * cpad), Guarded((B, N, F), torch.bfloat16, dev, PAD * F)
        tgt = c["tgt"] if (loss or border) else None
        state = [L.ptr(c["prev"]), N * F, L.ptr(tgt), N * F, L.ptr(c["std"]), L.ptr(c["mean"]), L.ptr(c["border"]), L.ptr(c["interior"]),
                 L.ptr(ns.t), N * F]
        if loss:
            L.call("p4c_out_conv_update_loss_fwd", *front, *state, L.ptr(c["weights"]), float(c["interior"].sum()), None, kcode,
                   L.ptr(lossv.t), 1, L.ptr(ws.t), B, N, F, 1.0, L.ptr(xn.t), *nxt, L.ptr(lgr.t), N * F, st)
        else:
            L.call("p4c_out_conv_update_fwd", *front, *state, B, N, F, 1.0, L.ptr(xn.t), *nxt, st)
        torch.cuda.synchronize()
        _check_guards(ns, lossv, ws, xn, lgr)
        tag = f"out_conv F={F} {'loss' if loss else 'free'}"
        _check_state(tag, c, cfg, ns, free=not loss)
        out, _, _ = _step_reference(c, cfg, ns.t, loss=loss, with_next=True)
        _same_bits(f"{tag} next input", xn.t, out["x_next"])
        if loss:
            _close(f"{tag} loss", lossv.t, out["loss"].detach(), 1e-5)
            _close(f"{tag} saved loss gradient (bf16)", lgr.t, out["lgrad"], BF16_RND)
