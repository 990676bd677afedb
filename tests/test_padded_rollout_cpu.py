"""
The float64 restatements of the window kernels (tests/padded_rollout_reference.py) proven on the CPU: composed over T = 2 with a
pad -> network -> crop model they are the oracle rollout (oracle/rollout.py) around oracle/halfunet.py applied as pad -> ref -> crop,
for both strategies, with and without NaNs; their gradients are autograd's through pad and crop.  And the routing predicate
(halfunet_rollout.padded_grid_is_native) answers as its restatement for every excluded case.
"""
import itertools

import padded_rollout_reference as P
import pytest
import step_reference as S
import torch
import torch.nn.functional as Fn


def _case(H, W, nan, border, T=2, F=6):
    from helpers import synthetic_case

    case = synthetic_case(seed=11, B=2, T=T, T_in=1, H=H, W=W, F=F, Ff=5, Fs=4, border=border)
    if nan:
        case["inputs"][0, 0, 3, 4, 1] = float("nan")
        case["forcing"][-1, -1, 5, 6, 2] = float("nan")
        case["outputs"][:, :, 7, 8, :] = float("nan")
        case["outputs"][0, -1, 2, 2, 0] = float("nan")
    return {k: v.double() for k, v in case.items()}


@pytest.mark.parametrize("H,W", [(33, 47), (40, 72)])
def test_geometry(H, W):
    g = P.geom(H, W)
    assert (g.Hp, g.Wp) == ((48, 48) if H == 33 else (48, 80))
    assert P.padding_for(33, 47) == (7, 8, 0, 1) and P.padding_for(40, 72) == (4, 4, 4, 4) and P.padding_for(64, 80) == (0, 0, 0, 0)
    x = torch.randn(2, H, W, 3, dtype=torch.float64)
    top, bottom, left, right = P.padding_for(H, W)
    padded = Fn.pad(x, (0, 0, left, right, top, bottom))
    assert torch.equal(P.pad_rows(x.reshape(2, H * W, 3), g), padded.reshape(2, g.Hp * g.Wp, 3))
    assert torch.equal(P.crop_rows(padded.reshape(2, -1, 3), g), x.reshape(2, H * W, 3))


@pytest.mark.parametrize("strategy", ["scaled_ar", "diff_ar"])
@pytest.mark.parametrize("nan,border", [(False, 2), (True, 0)])
def test_restatements_compose_to_the_oracle_rollout(strategy, nan, border):
    from oracle import losses as olosses
    from oracle import rollout as orollout
    from oracle.halfunet import HalfUNetRef

    H, W, T, F, B = 33, 47, 2, 6, 2
    g = P.geom(H, W)
    top, bottom, left, right = P.padding_for(H, W)
    c = _case(H, W, nan, border, T, F)
    c_in = F + 4 + 5 + int(nan)
    c_pad = c_in + 3
    torch.manual_seed(1)
    ref = HalfUNetRef(c_in, F).double().train()
    scale = strategy == "scaled_ar"
    std, mean = (c["diff_std"], c["diff_mean"]) if scale else (None, None)
    interior = 1.0 - c["border_mask"]
    statics = c["statics"].unsqueeze(0).expand(B, H, W, 4)
    wts = olosses.weighted_loss_weights(c["state_weight"], c["diff_std"], "mse")

    def padded_model(x):   # (B, C, H, W): the reference's AutoPaddingModel
        return ref(Fn.pad(x, (left, right, top, bottom)))[:, :, top:top + H, left:left + W]

    pred = orollout.rollout(padded_model, c["inputs"], c["forcing"], c["outputs"], statics, c["border_mask"], interior, std, mean,
                            strategy, 1, nan, "train", features_second=True)
    loss = olosses.training_loss(pred, c["outputs"], nan, [("WeightedLoss", 1.0, dict(weights=wts, interior_mask=interior, kind="mse"))])
    grads = torch.autograd.grad(loss, list(ref.parameters()))

    # the same rollout from the window restatements: the network sees rows of the padded grid and nothing is padded or cropped
    N = H * W
    flat = lambda t: t.reshape(B, N, -1)   # noqa: E731
    bm, im = c["border_mask"].reshape(N), interior.reshape(N)
    prev = flat(c["inputs"][:, 0])
    states, cols = [], []
    for i in range(T):
        x = P.build_x(prev, flat(statics), flat(c["forcing"][:, i]), g, c_pad, torch.float64, nan)
        assert float(x[..., c_in:].detach().abs().sum()) == 0.0
        y = ref(x[..., :c_in].reshape(B, g.Hp, g.Wp, c_in).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).reshape(B, g.Hp * g.Wp, F)
        out = P.fused_step(prev, y, flat(c["outputs"][:, i]), std, mean, bm if scale else None, im, wts, g, kind="mse", from_nan=nan)
        prev = out["new_state"]
        states.append(prev)
        cols.append(out["loss"])
    got = torch.stack(states, 1).reshape(B, T, H, W, F)
    assert torch.equal(torch.isnan(got), torch.isnan(pred))
    assert float((torch.nan_to_num(got) - torch.nan_to_num(pred)).abs().max()) < 1e-12
    # (the planted NaNs mask the same grid point in every column, so the per-column masked count is the reference's union count)
    got_loss = torch.stack(cols, 1).mean()
    assert abs(float(got_loss - loss)) / abs(float(loss)) < 1e-12
    got_grads = torch.autograd.grad(got_loss, list(ref.parameters()))
    for a, b in zip(got_grads, grads):
        assert float((a - b).abs().max()) <= 1e-10 * float(b.abs().max()) + 1e-300


@pytest.mark.parametrize("from_nan", [False, True])
def test_step_gradients_live_on_the_padded_grid(from_nan):
    """dy of the window step: autograd's gradient through the crop -- zero outside the window and in channels >= F; dx arrives as rows
    of the padded grid and only its window counts"""
    H, W, F, B, ycs = 33, 47, 6, 2, 8
    g = P.geom(H, W)
    c = _case(H, W, from_nan, 2, 1, F)
    N, NP = H * W, g.Hp * g.Wp
    gen = torch.Generator().manual_seed(2)
    y = torch.randn(B, NP, ycs, generator=gen, dtype=torch.float64).requires_grad_(True)
    prev = c["inputs"][:, 0].reshape(B, N, F).clone().requires_grad_(True)
    tgt = c["outputs"][:, 0].reshape(B, N, F)
    bm, im = c["border_mask"].reshape(N), (1.0 - c["border_mask"]).reshape(N)
    w = c["state_weight"]
    gl = torch.randn(B, generator=gen, dtype=torch.float64)
    gn = torch.randn(B, N, F, generator=gen, dtype=torch.float64)
    g2 = torch.randn(B, NP, ycs, generator=gen, dtype=torch.float64)
    out = P.fused_step(prev, y, tgt, c["diff_std"], c["diff_mean"], bm, im, w, g, from_nan=from_nan)
    dy, dprev = P.fused_step_grads(out, y, prev, g, gloss=gl, g_next=gn, g_next2=g2)
    inside = torch.zeros(NP, dtype=torch.bool)
    inside[P.window_rows(g)] = True
    assert float(dy[:, ~inside].abs().sum()) == 0.0 and float(dy[..., F:].abs().sum()) == 0.0
    # against the dense step fed the cropped rows
    yc = P.crop_rows(y.detach(), g).requires_grad_(True)
    pc = prev.detach().clone().requires_grad_(True)
    ref = S.fused_step(pc, yc, tgt, c["diff_std"], c["diff_mean"], bm, im, w, from_nan=from_nan)
    dyc, dpc = S.fused_step_grads(ref, yc, pc, gloss=gl, g_next=gn, g_next2=P.crop_rows(g2, g))
    assert torch.equal(P.crop_rows(dy, g), dyc) and torch.equal(dprev, dpc)
    assert torch.equal(torch.nan_to_num(out["new_state"]), torch.nan_to_num(ref["new_state"]))
    assert torch.equal(P.ar_update(prev, y, g, border_state=tgt, std=c["diff_std"], mean=c["diff_mean"], border_mask=bm, interior_mask=im,
                                   nan_to_num=from_nan).detach().nan_to_num(), out["new_state"].detach().nan_to_num())


def test_routing_predicate():
    from py4cast_amd.halfunet_rollout import padded_grid_is_native

    pads = [(7, 8, 0, 1), (4, 4, 4, 4), (0, 0, 0, 1), (0, 0, 0, 0)]
    for pad, autopad, T_in, K, channels in itertools.product(pads, (True, False), (1, 2), (1, 2), (21, 22)):
        assert padded_grid_is_native(pad, autopad, T_in, K, channels, 21) == P.routes_natively(pad, autopad, T_in, K, channels, 21)
    # the shipped configuration on the reference's own grids
    assert padded_grid_is_native(P.padding_for(717, 1121), True, 1, 1, 21, 21)
    # each excluded case
    assert not padded_grid_is_native((7, 8, 0, 1), False, 1, 1, 21, 21)   # autopad_enabled: False -> forward raises, generic route
    assert not padded_grid_is_native((7, 8, 0, 1), True, 2, 1, 21, 21)    # T_in >= 2
    assert not padded_grid_is_native((7, 8, 0, 1), True, 1, 2, 21, 21)    # num_inter_steps >= 2
    assert not padded_grid_is_native((7, 8, 0, 1), True, 1, 1, 22, 21)    # channel count
    assert not padded_grid_is_native((0, 0, 0, 0), True, 1, 1, 21, 21)    # a grid that fits: not a padded route


def test_launch_arithmetic():
    """a second loop trip needs more pixels than blocks * waves * pixels-per-wave; the side chosen for the GPU test is the smallest"""
    for lanes, B, cus in ((4, 2, 256), (32, 2, 256), (16, 2, 256), (8, 2, 304)):
        side = P.two_trip_side(lanes, B, cus)
        assert side % 16 and P.win_trips(side * side, lanes, B, cus) == 2
        smaller = side - 1 if (side - 1) % 16 else side - 2
        assert P.win_trips(smaller * smaller, lanes, B, cus) == 1
