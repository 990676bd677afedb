"""
tests/step_reference.py proved on the CPU: its float64 references against the oracle (oracle/losses.py, oracle/rollout.py,
oracle/next_rows.py) and against the golden vectors of the unmodified reference under tests/golden/, its fused-step reference
against ar_update followed by weighted_loss, and its launch arithmetic against the block and trip counts of the table of
tests/test_loop_trips_gpu.py at 256 compute units.
"""
import os

import numpy as np
import pytest
import torch

import step_reference as R
from conftest import golden_files, load_golden
from helpers import synthetic_case
from oracle import losses as olosses
from oracle import next_rows as onext
from oracle import rollout as orollout

FILES = golden_files()


def _flat(t, lead):
    return t.reshape(*t.shape[:lead], -1, t.shape[-1])


def _masks(case, mode):
    """(target as handed to the reference, oracle mask, oracle target, explicit mask tensor or None)"""
    outputs = case["outputs"]
    omask, otgt = orollout.get_mask_on_nan(outputs, True)
    if mode == "none":
        return otgt, torch.ones_like(otgt), otgt, None
    if mode == "from_nan":
        return outputs, omask, otgt, None
    if mode == "f32":
        return otgt, omask.float(), otgt, omask.float()
    return otgt, omask, otgt, omask.to(torch.uint8)


@pytest.mark.parametrize("mode", R.MASK_MODES)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("F,border", [(60, 2), (5, 0), (130, 1)])
def test_loss_references_equal_the_oracle(kind, mode, F, border):
    case = synthetic_case(seed=31, H=12, W=10, F=F, border=border, nan=True)
    case = {k: v.double() for k, v in case.items()}
    pred = torch.randn(case["outputs"].shape, generator=torch.Generator().manual_seed(32), dtype=torch.float64)
    target, omask, otgt, mask = _masks(case, mode)
    interior = 1.0 - case["border_mask"]
    wts = olosses.weighted_loss_weights(case["state_weight"], case["diff_std"], kind)
    clim = case["diff_mean"]
    fl = lambda t: None if t is None else _flat(t, 2)
    args = dict(kind=kind, mode=mode, mask=fl(mask))
    tol = dict(rtol=1e-12, atol=1e-12)
    got = R.weighted_loss(fl(pred), fl(target), wts, interior.reshape(-1), **args)
    np.testing.assert_allclose(got.numpy(), olosses.weighted_loss(pred, otgt, omask, wts, interior, kind).numpy(), **tol)
    got = R.weighted_loss_map(fl(pred), fl(target), wts, **args)
    ref = olosses.weighted_loss(pred, otgt, omask, wts, interior, kind, reduce_spatial_dim=False)
    np.testing.assert_allclose(got.numpy(), _flat(ref.unsqueeze(-1), 2)[..., 0].numpy(), **tol)
    got = R.scaled_loss(fl(pred), fl(target), case["std"], interior.reshape(-1), **args)
    np.testing.assert_allclose(got.numpy(), olosses.scaled_loss(pred, otgt, omask, case["std"], interior, kind).numpy(), **tol)
    # the anomaly-correlation sums: the oracle's increment is mean_b(num / sqrt(pp * tt))
    s = R.acc_sums(fl(pred), fl(target), clim, mode=mode, mask=fl(mask))
    np.testing.assert_allclose((s[0] / torch.sqrt(s[1] * s[2])).mean(0).numpy(), onext.acc_update(pred, otgt, omask, clim).numpy(), **tol)
    assert R.masked_count(fl(target), mode, fl(mask)) == int((~torch.any(omask != 0, dim=(0, 1, 4))).sum())


def test_weighted_loss_gradient_equals_the_oracle():
    case = {k: v.double() for k, v in synthetic_case(seed=33, H=9, W=11, F=21, border=1, nan=True).items()}
    interior = 1.0 - case["border_mask"]
    for kind in R.KINDS:
        wts = olosses.weighted_loss_weights(case["state_weight"], case["diff_std"], kind)
        p0 = torch.randn(case["outputs"].shape, generator=torch.Generator().manual_seed(34), dtype=torch.float64)
        gsel = torch.randn(p0.shape[:2], generator=torch.Generator().manual_seed(35), dtype=torch.float64)
        omask, otgt = orollout.get_mask_on_nan(case["outputs"], True)
        a, b = p0.clone().requires_grad_(True), p0.clone().requires_grad_(True)
        (olosses.weighted_loss(a, otgt, omask, wts, interior, kind) * gsel).sum().backward()
        (R.weighted_loss(_flat(b, 2), _flat(case["outputs"], 2), wts, interior.reshape(-1), kind, "from_nan") * gsel).sum().backward()
        np.testing.assert_allclose(b.grad.numpy(), a.grad.numpy(), rtol=1e-12, atol=1e-15)


def test_nan_moments_reference_equals_the_oracle():
    g = torch.Generator().manual_seed(36)
    x = torch.randn(3, 4, 7, 5, generator=g, dtype=torch.float64)
    x[0, 1, 2, 3] = float("nan")
    x[2, :, :, 0] = float("nan")
    xn = torch.randn(3, 4, 7, 5, generator=g, dtype=torch.float64)
    for a, b in ((x, None), (x, xn)):
        got, ref = R.nan_moments(a, b), onext.nan_moments(a, b).double()
        np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-6)      # (the oracle returns fp32)
        assert torch.equal(got[2], ref[2])


@pytest.mark.parametrize("scaled,border,nan", [(True, 2, False), (True, 1, True), (False, 0, False), (False, 0, True)])
def test_element_references_equal_the_oracle(scaled, border, nan):
    """ar_update against the body of oracle.rollout.rollout (one step of a one-layer 'model' that returns a fixed y), build_x against
    oracle.rollout.next_x: float64 to 1e-12, and the fp32 chain bit for bit."""
    case = synthetic_case(seed=37, B=2, T=2, T_in=2, H=9, W=10, F=5, Ff=3, Fs=4, border=border, nan=nan)
    B = 2
    statics = case["statics"].unsqueeze(0).expand(B, *case["statics"].shape)
    y32 = torch.randn(B, 9, 10, 5, generator=torch.Generator().manual_seed(38))
    for dt in (torch.float64, torch.float32):
        c = {k: v.to(dt) for k, v in case.items()}
        y = y32.to(dt)
        strategy = "scaled_ar" if scaled else "diff_ar"
        ref = orollout.rollout(lambda x: y, c["inputs"], c["forcing"], c["outputs"], statics.to(dt), c["border_mask"],
                               1.0 - c["border_mask"], c["diff_std"], c["diff_mean"], strategy, 1, nan)[:, 0]
        bm = c["border_mask"].reshape(-1)
        got = R.ar_update(_flat(c["inputs"][:, -1], 1), _flat(y, 1), _flat(c["outputs"][:, 0], 1) if scaled else None,
                          c["diff_std"] if scaled else None, c["diff_mean"] if scaled else None, bm if scaled else None,
                          (1.0 - bm) if scaled else None, 1.0, nan, dtype=dt)
        if dt == torch.float32:
            assert torch.equal(torch.nan_to_num(got, nan=9e9), torch.nan_to_num(_flat(ref, 1), nan=9e9))
        else:
            np.testing.assert_allclose(got.numpy(), _flat(ref, 1).numpy(), rtol=1e-12, atol=1e-12)
    ref = orollout.next_x(case["inputs"], statics, case["forcing"][:, 0], 2, mask_on_nan=nan)
    got = R.build_x(_flat(case["inputs"], 2), _flat(statics, 1), _flat(case["forcing"][:, 0], 1), mask_on_nan=nan)
    assert torch.equal(got, _flat(ref, 1).float())
    pad = R.build_x(_flat(case["inputs"], 2), _flat(statics, 1), _flat(case["forcing"][:, 0], 1), c_pad=32, out_dtype=torch.bfloat16,
                    mask_on_nan=nan)
    assert torch.equal(pad[..., : ref.shape[-1]], _flat(ref, 1).bfloat16()) and float(pad[..., ref.shape[-1]:].abs().sum()) == 0.0
    x = torch.randn(4, 9, 5, generator=torch.Generator().manual_seed(39))
    assert torch.equal(R.unnormalize(x, case["std"], case["diff_mean"], dtype=torch.float32),
                       onext.unnormalize(x, case["std"], case["diff_mean"]))


@pytest.mark.parametrize("path", [f for f in FILES if "grid" in f], ids=lambda p: p.split("/")[-1][:-4])
def test_loss_references_reproduce_the_golden_fixtures(path):
    """The unmodified reference's prediction as the operand: its four losses and the loss map at the bars of
    test_oracle_golden.py::test_losses_match_reference (rtol 2e-6, atol 1e-7); the NaN mask bit for bit."""
    meta, ins, outs = load_golden(path)
    t = {k: torch.from_numpy(v) for k, v in ins.items()}
    pred, outputs = torch.from_numpy(outs["prediction"]), t["outputs"]
    mode = "from_nan" if meta["nan"] else "none"
    m, _ = R.resolve_mask(outputs, mode)
    np.testing.assert_array_equal(m.numpy().astype(np.float32), outs["mask"])
    interior = (1.0 - t["border_mask"]).reshape(-1)
    fl = lambda x: _flat(x, 2)
    for tag, kind in (("wmse", "mse"), ("wl1", "l1")):
        wts = olosses.weighted_loss_weights(t["state_weight"], t["diff_std"], kind)
        val = R.weighted_loss(fl(pred), fl(outputs), wts, interior, kind, mode)
        vmap = R.weighted_loss_map(fl(pred), fl(outputs), wts, kind, mode)
        np.testing.assert_allclose(val.numpy(), outs[f"loss_{tag}"], rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(vmap.reshape(outs[f"loss_{tag}_map"].shape).numpy(), outs[f"loss_{tag}_map"], rtol=2e-6, atol=1e-7)
    for tag, kind in (("smse", "mse"), ("sl1", "l1")):
        val = R.scaled_loss(fl(pred), fl(outputs), t["std"], interior, kind, mode)
        np.testing.assert_allclose(val.numpy(), outs[f"loss_{tag}"], rtol=2e-6, atol=1e-7)


def test_row_references_reproduce_the_golden_fixtures():
    """next_acc.npz (bars of test_oracle_acc_matches_reference: rtol 1e-6, atol 1e-7), next_unnormalize.npz (bit for bit)."""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "next_acc.npz"), allow_pickle=False)
    clim = torch.from_numpy(z["clim"])
    total = None
    for step in range(2):
        p, g, m = (torch.from_numpy(z[f"{k}{step}"]) for k in ("pred", "target", "mask"))
        s = R.acc_sums(_flat(p, 2), _flat(g, 2), clim, mode="f32", mask=_flat(m.float().expand_as(p), 2))
        inc = (s[0] / torch.sqrt(s[1] * s[2])).mean(0)
        total = inc if total is None else total + inc
        np.testing.assert_allclose(total.numpy(), z[f"sum_acc{step}"], rtol=1e-6, atol=1e-7)
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "next_unnormalize.npz"), allow_pickle=False)
    out = R.unnormalize(torch.from_numpy(z["x"]), torch.from_numpy(z["std"]), torch.from_numpy(z["mean"]), dtype=torch.float32)
    assert np.array_equal(out.numpy(), z["out"])


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("scaled,border,nan,keep", [(True, True, False, 1.0), (True, True, True, 1.0), (False, False, False, 1.0),
                                                    (True, False, False, 0.0)])
def test_fused_step_reference_equals_update_then_loss(kind, scaled, border, nan, keep):
    g = torch.Generator().manual_seed(40)
    B, N, F, ycs = 2, 45, 12, 16
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    prev, y, tgt = rn(B, N, F), rn(B, N, ycs), rn(B, N, F)
    if nan:
        tgt[:, 7] = float("nan")
        tgt[0, 3, 2] = float("nan")
        prev[1, 5, 1] = float("nan")
    std, mean = (ru(F) + 0.5, rn(F) * 0.01) if scaled else (None, None)
    interior = (ru(N) > 0.2).double()
    bmask = 1.0 - interior
    w = ru(F) + 0.5
    statics, forcing = ru(B, N, 4), ru(B, N, 3)
    yl, pl = y.clone().requires_grad_(True), prev.clone().requires_grad_(True)
    out = R.fused_step(pl, yl, tgt, std, mean, bmask if border else None, interior, w, kind, keep, nan,
                       next_input=(statics, forcing, 24, torch.float64))
    ya, pa = y.clone().requires_grad_(True), prev.clone().requires_grad_(True)
    ns = R.ar_update(pa, ya, tgt if border else None, std, mean, bmask if border else None, interior if border else None, keep, nan)
    loss = R.weighted_loss(ns.unsqueeze(1), tgt.unsqueeze(1), w, interior, kind, "from_nan" if nan else "none")[:, 0]
    assert torch.equal(out["new_state"], ns)
    np.testing.assert_allclose(out["loss"].detach().numpy(), loss.detach().numpy(), rtol=1e-13)
    assert torch.equal(out["x_next"], R.build_x(ns.detach().unsqueeze(1), statics, forcing, 24, torch.float64))
    gloss, g1, g2 = ru(B) + 0.5, rn(B, N, F), rn(B, N, ycs)
    dy, dprev = R.fused_step_grads(out, yl, pl, gloss, g1, g2)
    ((gloss * loss).sum() + ((g1 + g2[..., :F]) * ns).sum()).backward()
    np.testing.assert_allclose(dy.numpy(), ya.grad.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(dprev.numpy(), pa.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert float(dy[..., F:].abs().max()) == 0.0
    # the saved loss gradient is d loss_elem / d pred, and the backward from it is the backward
    yb, pb = y.clone().requires_grad_(True), prev.clone().requires_grad_(True)
    out2 = R.fused_step(pb, yb, tgt, std, mean, bmask if border else None, interior, w, kind, keep, nan)
    dy2, dprev2 = R.fused_step_grads(out2, yb, pb, gloss, g1, g2, interior_mask=interior, weights=w, lgrad=out2["lgrad"])
    np.testing.assert_allclose(dy2.numpy(), dy.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(dprev2.numpy(), dprev.numpy(), rtol=1e-12, atol=1e-15)
    # a free step: the same state, no loss
    free = R.fused_step(prev, y, tgt if border else None, std, mean, bmask if border else None, interior if border else None, None, kind,
                        keep, nan, loss=False)
    assert torch.equal(free["new_state"], ns.detach()) and free["loss"] is None and free["lgrad"] is None


# ---- launch arithmetic at 256 compute units: the table of tests/test_loop_trips_gpu.py
CUS = 256


def test_launch_arithmetic_primitives():
    assert [R.pow2_ge64(v) for v in (1, 2, 3, 5, 15, 16, 21, 60, 64, 65, 256)] == [1, 2, 4, 8, 16, 16, 32, 64, 64, 64, 64]
    assert R.loss_blocks(480, 1, 6, CUS) == 120                    # the small-grid tests: 120 blocks against a cap of 342, one trip
    assert R.loss_trips(480, 60, 6, CUS) == 1
    assert R.loss_blocks(1517, 1, 6, CUS) == 342 and 1517 - 4 * 342 == 149
    assert R.loss_blocks(2491, 1, 1, CUS) == 512 == R.LOSS_MAX_BLOCKS
    assert R.loss_blocks(2491, 1, 2, CUS) == 512
    assert R.loss_blocks(12827, 8, 6, CUS) == 342 and 12827 % 8 == 3
    assert R.loss_blocks(36863, 64, 16, CUS) == 128
    assert R.mask_count_blocks(8827, 60, CUS) == 2048
    assert R.stream_grid(9514, 1, CUS) == 2048 and R.stream_grid(100, 1, CUS) == 25
    assert R.loss_blocks(8827, 4, 2, CUS) == 512                   # the 16-byte step at F = 60: 4 points per wave
    assert R.loss_blocks(8192, 4, 2, CUS) == 512 and R.step_v4_trips(8192, 60, 2, CUS) == 1     # "binds only above 8192 points"
    assert R.flat_blocks(36860, 2, CUS) == 512 and -(-36860 // 64) == 576 and 36860 % 64 == 60
    assert R.flat_blocks(32768, 2, CUS) == 512 and R.step_flat_trips(32768, 2, CUS) == 1        # "binds above 32768 points at B = 2"
    assert R.flat_blocks(1000, 1, CUS) == 16                       # fewer tiles than blocks: one block per tile
    assert R.trips(10, 3, 2) == 2 and R.trips(12, 3, 2) == 2 and R.trips(13, 3, 2) == 3


def test_every_tabled_case_takes_a_second_trip_at_256_cus():
    import test_loop_trips_gpu as G

    seen = 0
    for name, fn, args in G.tabled_trips():
        assert fn(*args, CUS) >= 2, (name, args)
        seen += 1
    assert seen >= 40
    # and the single-trip shapes the small-grid tests run really are single-trip
    assert R.step_v4_trips(6144, 60, 2, CUS) == 1 and R.step_flat_trips(6144, 2, CUS) == 1 and R.loss_trips(480, 60, 6, CUS) == 1
