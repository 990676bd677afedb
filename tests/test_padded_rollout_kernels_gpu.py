"""
The four window kernels of csrc/rollout_win.hip (the AR step of a rollout on an auto-padded grid), entry point by entry point:
  * every element of the network-side outputs (x, dy) is written -- the buffers start out as a sentinel -- and equals the restatement
    (tests/padded_rollout_reference.py) bit for bit: the existing kernel's values inside the window, +0.0 outside and in the
    channels past F;
  * the state-side outputs (new state, dprev) equal the existing kernels fed the cropped, contiguous rows bit for bit, and the guard
    regions on both sides of them stay untouched;
  * the loss column is within the `loss` bar of tests/rollout_nodes.py::BARS_F32 of float64;
  * a window that does not fit, or T_in = 2, returns the error code and launches nothing.
Grids: 33 x 47 -> 48 x 48 (asymmetric: top 7, bottom 8, left 0, right 1) and 40 x 72 -> 48 x 80 (4 each side): the smallest where a
wrong origin, swapped top / left, a pitch of W for Wp or an off-by-one at the far edge each show; and one grid per kernel form whose
size, derived from the kernels' own grid rule, takes a wave through a second pass of its loop.
"""
import padded_rollout_reference as P
import pytest
import step_reference as S
import torch

pytestmark = pytest.mark.gpu

SENT = 7.0
GUARD = 64     # elements (a multiple of 4: the guarded part stays 16-byte aligned)
LOSS_BAR = 1e-5   # tests/rollout_nodes.py::BARS_F32["loss"]
B, Fs, Ff, YCS = 2, 4, 5, 64


class Guarded:
    """``shape`` elements of the sentinel between two guard regions of the sentinel"""

    def __init__(self, shape, dtype, dev):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.n = n

    def intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.n:] == SENT).all())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    """bit-equal, NaN payloads aside (a NaN equals a NaN)"""
    return bool(((bits(a) == bits(b)) | (torch.isnan(a) & torch.isnan(b))).all())


def make_case(H, W, F, nan, dt, dev, seed=0, ycs=YCS):
    g = P.geom(H, W)
    N, NP = H * W, g.Hp * g.Wp
    gen = torch.Generator().manual_seed(seed + H * W + F)
    rn = lambda *s: torch.randn(*s, generator=gen)   # noqa: E731
    c = dict(prev=rn(B, N, F), tgt=rn(B, N, F), statics=torch.rand(B, N, Fs, generator=gen), forcing=torch.rand(B, N, Ff, generator=gen),
             y=rn(B, NP, ycs).to(dt), dx=rn(B, NP, ycs).to(dt), g_next=rn(B, N, F), gloss=rn(B), std=torch.rand(F, generator=gen) + 0.5,
             mean=rn(F) * 0.01, weights=torch.rand(F, generator=gen) + 1.0)
    border = torch.zeros(H, W)
    border[:2], border[-2:], border[:, :2], border[:, -2:] = 1, 1, 1, 1
    c["border"], c["interior"] = border.reshape(N), 1.0 - border.reshape(N)
    if nan:
        c["prev"][0, 3 * W + 4, 1] = float("nan")
        c["forcing"][-1, 5 * W + 6, 2] = float("nan")
        c["tgt"][:, 7 * W + 8, :] = float("nan")
        c["tgt"][0, 2 * W + 2, 0] = float("nan")
        c["tgt"][1, N - 1, F - 1] = float("nan")     # the far corner of the window
    c = {k: v.to(dev) for k, v in c.items()}
    c.update(g=g, N=N, NP=NP, F=F, nan=nan, dt=dt, dev=dev, ycs=ycs)
    return c


def win_args(g):
    return (g.H, g.W, g.Hp, g.Wp, g.top, g.left)


def check_build_x(c, cpad):
    from py4cast_amd import _lib as L

    g, N, NP, F, dev, dt = c["g"], c["N"], c["NP"], c["F"], c["dev"], c["dt"]
    st = L.stream(dev)
    x = Guarded((B, NP, cpad), dt, dev)
    head = (L.ptr(c["prev"]), N * F, N * F, L.ptr(c["statics"]), N * Fs, L.ptr(c["forcing"]), N * Ff)
    dims = (L.dtype_code(dt), cpad, B, 1, N, F, Fs, Ff, int(c["nan"]), 0)
    L.call("p4c_build_x_win", *head, L.ptr(x.t), *dims, *win_args(g), st)
    dense = torch.full((B, N, cpad), SENT, dtype=dt, device=dev)
    L.call("p4c_build_x", *head, L.ptr(dense), *dims, st)
    assert x.intact()
    assert same_bits(x.t, P.pad_rows(dense, g)), "x differs from p4c_build_x's rows inside the window or is not +0.0 outside"
    assert same_bits(x.t, P.build_x(c["prev"], c["statics"], c["forcing"], g, cpad, dt, c["nan"])), "x differs from the restatement"


def check_forward(c, kind, scaled, loss):
    from py4cast_amd import _lib as L

    g, N, NP, F, dev, dt, nan = c["g"], c["N"], c["NP"], c["F"], c["dev"], c["dt"], c["nan"]
    st = L.stream(dev)
    std, mean = (c["std"], c["mean"]) if scaled else (None, None)
    force = scaled
    yc = P.crop_rows(c["y"], g).contiguous()
    mode = L.MASK_FROM_NAN if nan else L.MASK_NONE
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    if nan:
        L.call("p4c_mask_all_zero_count", L.ptr(c["tgt"]), mode, N * F, N * F, B, 1, N, F, L.ptr(count), st)
    nint = float(c["interior"].sum())
    ws = torch.empty(L.lib().p4c_loss_workspace_bytes(B, 1, N, 1) // 4, dtype=torch.float32, device=dev)
    outs = {}
    for which, y in (("win", c["y"]), ("dense", yc)):
        ns = Guarded((B, N, F), torch.float32, dev)
        col = Guarded((B,), torch.float32, dev)
        target = c["tgt"] if (loss or force) else None
        state = (L.ptr(c["prev"]), N * F, L.ptr(y), L.dtype_code(dt), c["ycs"], L.ptr(target), N * F, L.ptr(std), L.ptr(mean),
                 L.ptr(c["border"] if force else None), L.ptr(c["interior"] if (loss or force) else None), L.ptr(ns.t), N * F)
        tail = win_args(g) if which == "win" else ()
        if loss:
            args = (*state, L.ptr(c["weights"]), nint, L.ptr(count), S.KINDS.index(kind), mode, L.ptr(col.t), 1, L.ptr(ws), B, N, F, 1.0)
            L.call("p4c_ar_update_loss_fwd_win" if which == "win" else "p4c_ar_update_loss_fwd", *args, *tail, st)
        elif which == "win":
            L.call("p4c_ar_update_next_win", *state, int(nan), B, N, F, 1.0, *tail, st)
        else:
            L.call("p4c_ar_update_next", *state, int(nan), B, N, F, 1.0, None, 0, None, 0, 0, None, 0, 0, st)
        assert ns.intact() and col.intact(), which
        outs[which] = (ns.t, col.t)
    assert same_bits(outs["win"][0], outs["dense"][0]), "new state differs from the existing kernel fed the cropped rows"
    assert not bool((outs["win"][0] == SENT).any()), "an element of the new state was not written"
    if loss:
        ref = S.fused_step(c["prev"], yc, c["tgt"], std, mean, c["border"] if force else None, c["interior"], c["weights"], kind=kind,
                           from_nan=nan, state=outs["win"][0])
        err = float(((outs["win"][1].double() - ref["loss"]).abs() / ref["loss"].abs()).max())
        print(f"loss column vs float64: {err:.3e}")
        assert err < LOSS_BAR
    else:
        assert bool((outs["win"][1] == SENT).all())
    return outs["win"][0], count


def check_backward(c, kind, scaled, ns, count, with_next):
    from py4cast_amd import _lib as L

    g, N, NP, F, dev, dt, nan = c["g"], c["N"], c["NP"], c["F"], c["dev"], c["dt"], c["nan"]
    st = L.stream(dev)
    std = c["std"] if scaled else None
    mode = L.MASK_FROM_NAN if nan else L.MASK_NONE
    nint = float(c["interior"].sum())
    dxc = P.crop_rows(c["dx"], g).contiguous()
    ycs = c["ycs"]
    outs = {}
    for which, dx, rows in (("win", c["dx"], NP), ("dense", dxc, N)):
        dy = Guarded((B, rows, ycs), dt, dev)
        dprev = Guarded((B, N, F), torch.float32, dev)
        args = (L.ptr(c["g_next"] if with_next else None), N * F, L.ptr(dx if with_next else None), L.dtype_code(dt), ycs, L.ptr(c["gloss"]), 1,
                L.ptr(ns), N * F, L.ptr(c["tgt"]), N * F, L.ptr(std), L.ptr(c["interior"]), int(scaled), L.ptr(c["weights"]), nint,
                L.ptr(count), S.KINDS.index(kind), mode, L.ptr(dy.t), L.dtype_code(dt), ycs, L.ptr(dprev.t), N * F, B, N, F, 1.0)
        if which == "win":
            L.call("p4c_ar_update_loss_bwd_win", *args, *win_args(g), st)
        else:
            L.call("p4c_ar_update_loss_bwd", *args, st)
        assert dy.intact() and dprev.intact(), which
        outs[which] = (dy.t, dprev.t)
    assert same_bits(outs["win"][0], P.pad_rows(outs["dense"][0], g)), "dy: not the existing kernel's rows inside the window, +0.0 elsewhere"
    assert float(outs["win"][0][..., F:].float().abs().sum()) == 0.0
    assert same_bits(outs["win"][1], outs["dense"][1]), "dprev differs from the existing kernel fed the cropped dx"
    if dt == torch.float32 and not nan:
        # and the float64 restatement itself: autograd through crop and step, the loss terms evaluated at the stored state
        y64 = c["y"].double().requires_grad_(True)
        p64 = c["prev"].double().requires_grad_(True)
        out = P.fused_step(p64, y64, c["tgt"], std, c["mean"] if scaled else None, c["border"] if scaled else None, c["interior"],
                           c["weights"], g, kind=kind, state=ns)
        dy64, dp64 = P.fused_step_grads(out, y64, p64, g, gloss=c["gloss"], g_next=c["g_next"] if with_next else None,
                                        g_next2=c["dx"] if with_next else None)
        for name, got, ref in (("dy", outs["win"][0], dy64), ("dprev", outs["win"][1], dp64)):
            err = float((got.double() - ref).abs().max() / ref.abs().max())
            print(f"{name} vs float64: {err:.3e}")
            assert err < 1e-5, name    # tests/rollout_nodes.py::BARS_F32 dy / dprev


def run_all(c, kind, cpad=32):
    scaled = kind == "mse"    # MSE with scaled_ar (std / mean, forced border), L1 with diff_ar (neither)
    check_build_x(c, cpad)
    ns, count = check_forward(c, kind, scaled, loss=True)
    check_forward(c, kind, scaled, loss=False)
    check_backward(c, kind, scaled, ns, count, with_next=True)
    check_backward(c, kind, scaled, ns, count, with_next=False)


@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("F", [12, 21])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W", [(33, 47), (40, 72)])
def test_window_kernels(gpu_device, H, W, dt, F, nan, kind):
    run_all(make_case(H, W, F, nan, dt, gpu_device), kind)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("F", [12, 21])
def test_rows_off_the_quad_grid(gpu_device, F, dt):
    """network rows of 23 channels: no 16-byte form applies to y, the lane-per-feature forward steps run at either F; the backward
    step, whose lanes own quads of a dy / dx row at every F, refuses such rows"""
    from py4cast_amd import _lib as L

    for (H, W, nan, kind) in ((33, 47, True, "mse"), (40, 72, False, "l1")):
        c = make_case(H, W, F, nan, dt, gpu_device, ycs=23)
        check_forward(c, kind, kind == "mse", loss=True)
        check_forward(c, kind, kind == "mse", loss=False)
    # the backward step on such rows: a case of its own, operands valid in every other respect
    c = make_case(33, 47, F, False, dt, gpu_device, ycs=23)
    g, N = c["g"], c["N"]
    new_state = torch.randn(B, N, F, device=gpu_device)
    dy = torch.full((B, c["NP"], 23), SENT, dtype=dt, device=gpu_device)
    rc = L.lib().p4c_ar_update_loss_bwd_win(None, N * F, None, L.dtype_code(dt), 23, L.ptr(c["gloss"]), 1, L.ptr(new_state), N * F,
                                            L.ptr(c["tgt"]), N * F, None, L.ptr(c["interior"]), 0, L.ptr(c["weights"]),
                                            float(c["interior"].sum()), None, L.LOSS_L1, L.MASK_NONE, L.ptr(dy), L.dtype_code(dt), 23, None,
                                            N * F, B, N, F, 1.0, *win_args(g), L.stream(gpu_device))
    torch.cuda.synchronize()
    assert rc == L.ERR_UNSUPPORTED and bool((dy == SENT).all())    # nothing launched


def test_free_step_without_a_target(gpu_device):
    """the forecast's free step: target / border / interior NULL together"""
    from py4cast_amd import _lib as L

    for F, dt in ((12, torch.bfloat16), (21, torch.float32)):
        c = make_case(33, 47, F, False, dt, gpu_device)
        g, N = c["g"], c["N"]
        st = L.stream(gpu_device)
        outs = []
        for win in (True, False):
            ns = Guarded((B, N, F), torch.float32, gpu_device)
            y = c["y"] if win else P.crop_rows(c["y"], g).contiguous()
            state = (L.ptr(c["prev"]), N * F, L.ptr(y), L.dtype_code(dt), YCS, None, 0, L.ptr(c["std"]), L.ptr(c["mean"]), None, None,
                     L.ptr(ns.t), N * F, 0, B, N, F, 1.0)
            if win:
                L.call("p4c_ar_update_next_win", *state, *win_args(g), st)
            else:
                L.call("p4c_ar_update_next", *state, None, 0, None, 0, 0, None, 0, 0, st)
            assert ns.intact()
            outs.append(ns.t)
        assert same_bits(outs[0], outs[1])


@pytest.mark.parametrize("F,nan", [(12, False), (21, True)])
def test_second_loop_trip(gpu_device, F, nan):
    """every window kernel caps its grid (blocks_per_sample) and strides; the grid is the smallest that takes each of the case's three
    kernel forms (build_x, forward step, backward step) through a second pass"""
    from py4cast_amd import _lib as L

    cus = L.lib().p4c_num_cus()
    cpad = 32
    lanes_fwd = S.pow2_ge64(F // 4) if F % 4 == 0 else S.pow2_ge64(F)
    lanes_x = S.pow2_ge64(cpad) if nan else S.pow2_ge64(cpad // 4)
    lanes_bwd = S.pow2_ge64(YCS // 4)    # rows of 64 channels: the quad form at every F
    # the form with the fewest lanes per pixel covers the most pixels per pass: its second pass needs the largest grid
    side = max(P.two_trip_side(lanes, B, cus) for lanes in (lanes_fwd, lanes_x, lanes_bwd))
    g = P.geom(side, side)
    assert P.win_trips(side * side, lanes_fwd, B, cus) >= 2
    assert P.win_trips(g.Hp * g.Wp, lanes_x, B, cus) >= 2 and P.win_trips(g.Hp * g.Wp, lanes_bwd, B, cus) >= 2
    run_all(make_case(side, side, F, nan, torch.float32, gpu_device), "mse", cpad)


def test_bad_arguments_return_the_error_code_and_launch_nothing(gpu_device):
    from py4cast_amd import _lib as L

    F, dt = 12, torch.float32
    c = make_case(33, 47, F, False, dt, gpu_device)
    g, N, NP = c["g"], c["N"], c["NP"]
    st = L.stream(gpu_device)
    lib = L.lib()
    x = torch.full((B, NP, 32), SENT, device=gpu_device)
    ns = torch.full((B, N, F), SENT, device=gpu_device)
    dy = torch.full((B, NP, YCS), SENT, device=gpu_device)
    col = torch.full((B,), SENT, device=gpu_device)
    ws = torch.empty(lib.p4c_loss_workspace_bytes(B, 1, N, 1) // 4, device=gpu_device)
    good = win_args(g)
    bad_windows = [
        (g.H, g.W, g.Hp, g.Wp, g.top + 9, g.left),      # top + H > Hp
        (g.H, g.W, g.Hp, g.Wp, g.top, g.left + 2),      # left + W > Wp
        (g.H, g.W, g.Hp, g.W - 1, g.top, 0),            # Wp < W
        (g.H, g.W, g.Hp, g.Wp, -1, g.left),             # negative origin
        (g.H + 1, g.W, g.Hp, g.Wp, g.top, g.left),      # H * W != N
    ]

    def build_x(win, T_in=1):
        return lib.p4c_build_x_win(L.ptr(c["prev"]), N * F, N * F, L.ptr(c["statics"]), N * Fs, L.ptr(c["forcing"]), N * Ff, L.ptr(x),
                                   L.F32, 32, B, T_in, N, F, Fs, Ff, 0, 0, *win, st)

    def fwd(win):
        return lib.p4c_ar_update_loss_fwd_win(L.ptr(c["prev"]), N * F, L.ptr(c["y"]), L.F32, YCS, L.ptr(c["tgt"]), N * F, L.ptr(c["std"]),
                                              L.ptr(c["mean"]), None, L.ptr(c["interior"]), L.ptr(ns), N * F, L.ptr(c["weights"]),
                                              float(c["interior"].sum()), None, 0, 0, L.ptr(col), 1, L.ptr(ws), B, N, F, 1.0, *win, st)

    def nxt(win):
        return lib.p4c_ar_update_next_win(L.ptr(c["prev"]), N * F, L.ptr(c["y"]), L.F32, YCS, None, 0, L.ptr(c["std"]), L.ptr(c["mean"]), None,
                                          None, L.ptr(ns), N * F, 0, B, N, F, 1.0, *win, st)

    def bwd(win):
        return lib.p4c_ar_update_loss_bwd_win(None, N * F, None, L.F32, YCS, L.ptr(c["gloss"]), 1, L.ptr(c["prev"]), N * F, L.ptr(c["tgt"]),
                                              N * F, L.ptr(c["std"]), L.ptr(c["interior"]), 0, L.ptr(c["weights"]),
                                              float(c["interior"].sum()), None, 0, 0, L.ptr(dy), L.F32, YCS, None, N * F, B, N, F, 1.0, *win, st)

    for win in bad_windows:
        for fn in (build_x, fwd, nxt, bwd):
            assert fn(win) == L.ERR_INVALID, (fn.__name__, win)
            assert lib.p4c_last_error()
    assert build_x(good, T_in=2) == L.ERR_INVALID
    torch.cuda.synchronize()
    for t in (x, ns, dy, col):
        assert bool((t == SENT).all()), "a refused call wrote to its output"
    assert build_x(good) == L.OK and fwd(good) == L.OK and nxt(good) == L.OK and bwd(good) == L.OK
    torch.cuda.synchronize()
    assert not bool((x == SENT).any()) and not bool((dy == SENT).any())
