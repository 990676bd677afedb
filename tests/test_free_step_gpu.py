"""
The loss-free AR step (an intermediary step of num_inter_steps >= 2, an inference step): p4c_ar_update_next, p4c_out_conv_update_fwd
and p4c_ar_update_next_bwd (csrc/losses.hip).  They are compile-time variants of the loss-carrying kernels, so their new state and
next input are pinned BIT FOR BIT to p4c_ar_update_loss_fwd[_next] / p4c_out_conv_update_loss_fwd (themselves pinned to the reference:
tests/test_rollout_gpu.py, test_flat_step_gpu.py, test_fused_tail_gpu.py) and, without a target, to ops.ar_update; the backward is
checked against the closed form in float64.

Paths by (N, F): (1536, 12), (1536, 60) 16-byte; (1536, 21) flat; (391, 12) N no multiple of any tile (16-byte); (391, 21) N * F % 4 != 0:
scalar.  The scalar path emits no next input -- neither does p4c_ar_update_loss_fwd_next there (P4C_ERR_UNSUPPORTED, the rollout runs
p4c_build_x) -- so for that shape the x_next case asserts the refusal of both and compares the state without it.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1536, 12), (1536, 60), (1536, 21), (391, 12), (391, 21)]
B, FS, FF = 2, 4, 5


def _scalar_only(N, F):
    return F % 4 != 0 and (N * F) % 4 != 0


def _cpad(F, bf16):
    return 96 if (F != 60 or bf16) else 72


def _case(dev, N, F, bf16, scaled, seed=11):
    g = torch.Generator(device=dev).manual_seed(seed + N + F)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    ru = lambda *s: torch.rand(*s, generator=g, device=dev)
    y = rn(B, N, 64)
    c = dict(prev=rn(B, N, F), tgt=rn(B, N, F), y=y.bfloat16() if bf16 else y, weights=ru(F) + 0.5,
             std=(ru(F) + 0.5) if scaled else None, mean=(rn(F) * 0.01) if scaled else None,
             interior=(ru(N) > 0.2).float(), statics=ru(B, N, FS), forcing=ru(B, N, FF))
    c["border"] = 1.0 - c["interior"]
    return c


def _loss_step(L, c, N, F, border, xn, cpad):
    """The loss-carrying step on the same inputs: (new_state, x_next)."""
    dev = c["prev"].device
    ns, loss = torch.full((B, N, F), 5.0, device=dev), torch.empty(B, device=dev)
    ws = torch.empty(L.lib().p4c_loss_workspace_bytes(B, 1, N, 1) // 4, dtype=torch.float32, device=dev)
    args = [L.ptr(c["prev"]), N * F, L.ptr(c["y"]), L.dtype_code(c["y"].dtype), 64, L.ptr(c["tgt"]), N * F, L.ptr(c["std"]), L.ptr(c["mean"]),
            L.ptr(c["border"] if border else None), L.ptr(c["interior"]), L.ptr(ns), N * F, L.ptr(c["weights"]), float(c["interior"].sum()),
            None, 0, L.MASK_NONE, L.ptr(loss), 1, L.ptr(ws), B, N, F, 1.0]
    if xn is not None:
        L.call("p4c_ar_update_loss_fwd_next", *args, L.ptr(xn), cpad, L.ptr(c["statics"]), N * FS, FS, L.ptr(c["forcing"]), N * FF, FF,
               L.stream(dev))
    else:
        L.call("p4c_ar_update_loss_fwd", *args, L.stream(dev))
    return ns, xn


def _free_step(L, c, N, F, target, border, interior, xn, cpad, nan_to_num=0, prev=None):
    dev = c["prev"].device
    ns = torch.full((B, N, F), 9.0, device=dev)
    L.call("p4c_ar_update_next", L.ptr(c["prev"] if prev is None else prev), N * F, L.ptr(c["y"]), L.dtype_code(c["y"].dtype), 64,
           L.ptr(target), N * F, L.ptr(c["std"]), L.ptr(c["mean"]), L.ptr(border), L.ptr(interior), L.ptr(ns), N * F, nan_to_num, B, N, F,
           1.0, L.ptr(xn), cpad, L.ptr(c["statics"]), N * FS, FS, L.ptr(c["forcing"]), N * FF, FF, L.stream(dev))
    return ns


def _xbuf(dev, N, cpad, bf16):
    x = torch.full((B, N, cpad), 7.0, device=dev)
    return x.bfloat16() if bf16 else x


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("nxt", [False, True])
@pytest.mark.parametrize("scaled", [True, False])
@pytest.mark.parametrize("border", [True, False])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("N,F", SHAPES)
def test_free_step_equals_the_loss_carrying_step(gpu_device, N, F, bf16, border, scaled, nxt):
    """Same inputs, arbitrary target and weights: new state and next input bit for bit; a second launch gives the same bits."""
    from py4cast_amd import _lib as L

    dev = gpu_device
    c = _case(dev, N, F, bf16, scaled)
    cpad = _cpad(F, bf16)
    tgt, bm, im = (c["tgt"], c["border"], c["interior"]) if border else (None, None, None)
    if nxt and _scalar_only(N, F):
        with pytest.raises(L.P4CError):
            _loss_step(L, c, N, F, border, _xbuf(dev, N, cpad, bf16), cpad)
        with pytest.raises(L.P4CError):
            _free_step(L, c, N, F, tgt, bm, im, _xbuf(dev, N, cpad, bf16), cpad)
        nxt = False
    ns0, xn0 = _loss_step(L, c, N, F, border, _xbuf(dev, N, cpad, bf16) if nxt else None, cpad)
    xn1 = _xbuf(dev, N, cpad, bf16) if nxt else None
    ns1 = _free_step(L, c, N, F, tgt, bm, im, xn1, cpad)
    xn2 = _xbuf(dev, N, cpad, bf16) if nxt else None
    ns2 = _free_step(L, c, N, F, tgt, bm, im, xn2, cpad)
    torch.cuda.synchronize()
    assert torch.equal(ns1, ns0), float((ns1 - ns0).abs().max())
    assert torch.equal(ns2, ns1)
    if nxt:
        assert torch.equal(_bits(xn1), _bits(xn0))
        assert torch.equal(_bits(xn2), _bits(xn1))


@pytest.mark.parametrize("nxt", [False, True])
@pytest.mark.parametrize("scaled", [True, False])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("N,F", SHAPES)
def test_free_step_without_target_equals_ar_update(gpu_device, N, F, bf16, scaled, nxt):
    """The inference form: target, border and interior masks all NULL.  The next input's state channels are the new state."""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    dev = gpu_device
    c = _case(dev, N, F, bf16, scaled, seed=17)
    cpad = _cpad(F, bf16)
    nxt = nxt and not _scalar_only(N, F)
    ref = ops.ar_update(c["prev"], c["y"], None, c["std"], c["mean"], None, None, keep_prev=1.0)
    xn = _xbuf(dev, N, cpad, bf16) if nxt else None
    ns = _free_step(L, c, N, F, None, None, None, xn, cpad)
    ns2 = _free_step(L, c, N, F, None, None, None, None, cpad)
    torch.cuda.synchronize()
    assert torch.equal(ns, ref), float((ns - ref).abs().max())
    assert torch.equal(ns2, ns)
    if nxt:
        want = torch.cat([ns, c["statics"], c["forcing"], torch.zeros(B, N, cpad - F - FS - FF, device=dev)], dim=-1).to(xn.dtype)
        assert torch.equal(_bits(xn), _bits(want))


@pytest.mark.parametrize("border", [True, False])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("N,F", SHAPES)
def test_free_step_nan_to_num_equals_ar_update(gpu_device, N, F, bf16, border):
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    dev = gpu_device
    c = _case(dev, N, F, bf16, True, seed=29)
    prev, tgt = c["prev"].clone(), c["tgt"].clone()
    prev[0, 3, 1] = float("nan")
    prev[1, N - 1, F - 1] = float("nan")
    border_pts = torch.nonzero(c["border"])[:, 0]
    tgt[:, border_pts[0], :] = float("nan")
    tgt[1, border_pts[-1], 0] = float("nan")
    tgt[0, 5, 2] = float("nan")
    bm, im = (c["border"], c["interior"]) if border else (None, None)
    ref = ops.ar_update(prev, c["y"], tgt if border else None, c["std"], c["mean"], bm, im, keep_prev=1.0, nan_to_num=True)
    ns = _free_step(L, c, N, F, tgt if border else None, bm, im, None, 0, nan_to_num=1, prev=prev)
    ns2 = _free_step(L, c, N, F, tgt if border else None, bm, im, None, 0, nan_to_num=1, prev=prev)
    torch.cuda.synchronize()
    assert not torch.isnan(ref).any()
    assert torch.equal(ns, ref), float((ns - ref).abs().max())
    assert torch.equal(ns2, ns)


@pytest.mark.parametrize("with_target", [True, False])
@pytest.mark.parametrize("nxt", [True, False])
@pytest.mark.parametrize("F,cpad", [(12, 96), (21, 96), (60, 96), (60, 100)])
def test_fused_output_conv_free_step_equals_the_loss_carrying_one(gpu_device, F, cpad, nxt, with_target):
    """p4c_out_conv_update_fwd against p4c_out_conv_update_loss_fwd (N = 32 * 48, cout = F).  Both entries select the same form: the
    flat one with the convolution as its front end wherever it applies; (60, 100) -- rows of the next input that are no whole
    16-byte slots -- is left to the 16-byte form when a next input is asked for.  Without a target: the same call with the border
    forcing off on both sides."""
    from py4cast_amd import _lib as L

    dev = gpu_device
    H, W = 32, 48
    N = H * W
    g = torch.Generator(device=dev).manual_seed(23 + F)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    ru = lambda *s: torch.rand(*s, generator=g, device=dev)
    a = rn(B, N, 64).bfloat16()
    sc, sh = ru(B, 64) + 0.5, rn(B, 64) * 0.3
    w = (rn(F, 64) * 0.2).contiguous()
    prev, tgt = rn(B, N, F), rn(B, N, F)
    std, mean = ru(F) + 0.5, rn(F) * 0.01
    interior = (ru(N) > 0.2).float()
    border = 1.0 - interior
    weights = ru(F) + 0.5
    statics, forcing = ru(B, N, FS), ru(B, N, FF)
    ws = torch.empty(L.lib().p4c_loss_workspace_bytes(B, 1, N, 1) // 4, dtype=torch.float32, device=dev)
    st = L.stream(dev)
    ns0, loss0 = torch.full((B, N, F), 5.0, device=dev), torch.empty(B, device=dev)
    xn0 = _xbuf(dev, N, cpad, True) if nxt else None
    L.call("p4c_out_conv_update_loss_fwd", L.ptr(a), L.ptr(sc), L.ptr(sh), L.ptr(w), F, L.ptr(prev), N * F, L.ptr(tgt), N * F,
           L.ptr(std), L.ptr(mean), L.ptr(border if with_target else None), L.ptr(interior), L.ptr(ns0), N * F, L.ptr(weights),
           float(interior.sum()), None, 0, L.ptr(loss0), 1, L.ptr(ws), B, N, F, 1.0, L.ptr(xn0), cpad, L.ptr(statics), N * FS, FS,
           L.ptr(forcing), N * FF, FF, None, 0, st)
    outs = []
    for _ in range(2):
        ns1 = torch.full((B, N, F), 9.0, device=dev)
        xn1 = _xbuf(dev, N, cpad, True) if nxt else None
        L.call("p4c_out_conv_update_fwd", L.ptr(a), L.ptr(sc), L.ptr(sh), L.ptr(w), F, L.ptr(prev), N * F,
               L.ptr(tgt if with_target else None), N * F, L.ptr(std), L.ptr(mean), L.ptr(border if with_target else None),
               L.ptr(interior if with_target else None), L.ptr(ns1), N * F, B, N, F, 1.0, L.ptr(xn1), cpad, L.ptr(statics), N * FS, FS,
               L.ptr(forcing), N * FF, FF, st)
        outs.append((ns1, xn1))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], ns0), float((outs[0][0] - ns0).abs().max())
    assert torch.equal(outs[1][0], outs[0][0])
    if nxt:
        assert torch.equal(_bits(outs[0][1]), _bits(xn0))
        assert torch.equal(_bits(outs[1][1]), _bits(outs[0][1]))


@pytest.mark.parametrize("force", [True, False])
@pytest.mark.parametrize("scaled", [True, False])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("N,F", SHAPES)
def test_free_step_backward_against_the_closed_form(gpu_device, N, F, bf16, scaled, force):
    """dy = ((g1 + g2) * interior) * std in the row dtype, dprev = (g1 + g2) * interior (keep_prev = 1); no interior factor where nothing
    is forced, and then dprev == g exactly.  Bounds: fp32 rows 1e-6 elementwise relative (two fp32 multiplications of <= 2^-24 each on
    top of one addition, a factor 8 of room); bf16 rows 4e-3 (one more rounding of 2^-9 -- the addend g2 is given in bf16 exactly)."""
    from py4cast_amd import _lib as L

    dev = gpu_device
    g = torch.Generator(device=dev).manual_seed(41 + N + F)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    dt = torch.bfloat16 if bf16 else torch.float32
    code = L.dtype_code(dt)
    g1 = rn(B, N, F)
    g2 = rn(B, N, 64).to(dt)
    std = (torch.rand(F, generator=g, device=dev) + 0.5) if scaled else None
    interior = (torch.rand(N, generator=g, device=dev) > 0.2).float()
    outs = []
    for _ in range(2):
        dy = torch.full((B, N, 64), 3.0, device=dev).to(dt)
        dprev = torch.full((B, N, F), 3.0, device=dev)
        L.call("p4c_ar_update_next_bwd", L.ptr(g1), N * F, L.ptr(g2), code, 64, L.ptr(std), L.ptr(interior if force else None), int(force),
               L.ptr(dy), code, 64, L.ptr(dprev), N * F, B, N, F, 1.0, L.stream(dev))
        outs.append((dy, dprev))
    torch.cuda.synchronize()
    dy, dprev = outs[0]
    assert torch.equal(_bits(outs[1][0]), _bits(dy)) and torch.equal(outs[1][1], dprev)
    gsum32 = g1 + g2[..., :F].float()
    gs = g1.double() + g2[..., :F].double()
    if force:
        gs = gs * interior.double()[None, :, None]
    ref_dy = gs * std.double() if scaled else gs
    tol = 4e-3 if bf16 else 1e-6
    got = dy[..., :F].double()
    err = ((got - ref_dy).abs() / ref_dy.abs().clamp_min(1e-30))[ref_dy != 0]
    print("max rel err dy", float(err.max()))
    assert float(err.max()) <= tol
    assert torch.equal(got[ref_dy == 0], torch.zeros_like(got[ref_dy == 0]))
    assert float(dy[..., F:].float().abs().max()) == 0.0
    errp = ((dprev.double() - gs).abs() / gs.abs().clamp_min(1e-30))[gs != 0]
    assert float(errp.max()) <= 1e-6
    if not force:
        assert torch.equal(dprev, gsum32)
    # g_next2 and dprev NULL: either addend and the state gradient are optional
    dy1 = torch.empty(B, N, 64, device=dev).to(dt)
    L.call("p4c_ar_update_next_bwd", L.ptr(g1), N * F, None, code, 64, L.ptr(std), L.ptr(interior if force else None), int(force),
           L.ptr(dy1), code, 64, None, N * F, B, N, F, 1.0, L.stream(dev))
    torch.cuda.synchronize()
    r1 = g1.double() * (interior.double()[None, :, None] if force else 1.0)
    r1 = r1 * std.double() if scaled else r1
    e1 = ((dy1[..., :F].double() - r1).abs() / r1.abs().clamp_min(1e-30))[r1 != 0]
    assert float(e1.max()) <= tol
