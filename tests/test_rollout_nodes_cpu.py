"""
The references of tests/rollout_nodes.py, on the CPU in float64 (no GPU, no product kernel).

Composition: the per-call references chained over the schedule of every case of the table (each call fed the previous call's reference
output, the reverse sweep from the per-call adjoints) reproduce oracle.rollout.rollout + oracle.losses.training_loss + backward() on the
same HalfUNetRef to 1e-10 relative -- prediction, loss, every parameter gradient, with the gradient injected at the prediction where
the case has one -- and the checker finds every node of that chain at zero.

Sensitivity: every wiring fact tests/test_rollout_nodes_gpu.py is meant to catch is planted in the chain as the device would show it;
the checker, which judges every node from the stored values upstream of it, must see the node named as its detector move by at least
10 x that node's bar (any difference at all where the bar is bit-equality).  Besides the schedule's wirings these cover the inside of
a model call (eval fed batch statistics, a middle block on another block's weights: the block nodes), the backward handed another
call's saved workspace (dx and p.grad) and the saved loss gradients stored one row off.
"""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rollout_nodes as RN  # noqa: E402

_CACHE = {}


def _chain(name, wrong=None):
    """the case's inputs, reference model and chain (the unplanted one is computed once per case)"""
    case = RN.CASES[name]
    if name not in _CACHE:
        c = RN.case_inputs(case)
        ref = RN.make_ref(case)
        _CACHE[name] = (c, ref, RN.chain(case, c, ref))
    c, ref, run = _CACHE[name]
    return case, c, ref, (run if wrong is None else RN.chain(case, c, ref, wrong=wrong))


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("name", list(RN.CASES))
def test_chain_of_per_call_references_is_the_oracle_rollout(name):
    from oracle import losses as olosses
    from oracle import rollout as orollout

    case, c, ref, run = _chain(name)
    forecast = case.mode == "forecast"
    c64 = {k: v.double() for k, v in c.items()}
    statics = c64["statics"].unsqueeze(0).expand(RN.B, *c64["statics"].shape)
    interior = 1.0 - c64["border_mask"]
    scaled = case.strategy == "scaled_ar"
    model = copy.deepcopy(ref)
    model.train(case.mode != "eval")
    pred = orollout.rollout(model, c64["inputs"], c64["forcing"], None if forecast else c64["outputs"], statics, c64["border_mask"], interior,
                            c64["diff_std"] if scaled else None, c64["diff_mean"] if scaled else None, case.strategy, case.K, case.nan,
                            "inference" if forecast else "train", features_second=True, num_pred_steps=case.T)
    assert _rel(run.pred, RN.rows4(pred.detach())) < 1e-10, "prediction"
    for k_, v in model.named_buffers():
        assert _rel(run.buffers[k_], v) < 1e-10 or float(v.double().abs().max()) == 0.0, k_
    if forecast:
        return
    wts = olosses.weighted_loss_weights(c64["state_weight"], c64["diff_std"], "mse")
    mask, tm = orollout.get_mask_on_nan(c64["outputs"], case.nan)
    per_bt = olosses.weighted_loss(pred, tm, mask, wts, interior, "mse")
    assert _rel(run.loss, per_bt.detach()) < 1e-10, "loss (B, T)"
    if case.mode != "train":
        return
    total = olosses.training_loss(pred, c64["outputs"], case.nan, [("WeightedLoss", RN.LOSS_WEIGHT, dict(weights=wts, interior_mask=interior, kind="mse"))])
    assert _rel(torch.mean(run.fused_loss), total.detach()) < 1e-10, "training loss"
    if case.gpred:
        total = total + RN.GPRED * (RN.rows4(pred) * RN.gpred_weights(case).double()).sum()
    total.backward()
    params = dict(model.named_parameters())
    assert set(params) == set(run.pgrads)
    for n, p in params.items():
        assert _rel(run.pgrads[n], p.grad) < 1e-10, f"gradient of {n}"


@pytest.mark.parametrize("name", list(RN.CASES))
def test_checker_finds_the_reference_chain_at_zero(name):
    """the checker recomputes every node of the chain from the chain's own records: nothing moves"""
    case, c, ref, run = _chain(name)
    fig = RN.check(run, ref)
    assert {"x", "prev", "slot", "pred"} <= {f[0] for f in fig}
    if case.mode == "train":
        assert {"dy", "pgrad", "sentinel", "gsum" if case.T_in > 1 else "gnext"} <= {f[0] for f in fig}
    for node, what, value, _ in fig:
        for v in (value if isinstance(value, tuple) else (value,)):
            assert v <= 1e-10, f"{name}: {what}: {node} {v:.3e}"


# (wrong wiring, case, the nodes that must see it)
SENSITIVITY = [
    ("free_forcing_next", "inter3-f32", ("x",)),
    ("free_forcing_next", "inter2-bf16", ("x",)),
    ("inter_to_pred", "inter3-f32", ("prev", "slot")),
    ("gsum_drop_block", "window-wrap-f32", ("gsum", "parts")),
    ("gsum_drop_block", "window-bf16", ("gsum", "parts")),
    ("gsum_offset_plus", "window-wrap-f32", ("gsum", "parts")),
    ("gsum_offset_minus", "window-wrap-f32", ("gsum", "parts")),
    ("gsum_offset_plus", "window-short-f32", ("gsum", "parts")),
    ("drop_dprev", "feed-f32", ("gnext",)),
    ("drop_dprev", "window-wrap-f32", ("gsum", "parts")),
    ("gpred_dropped", "gpred-f32", ("gnext",)),
    ("gpred_dropped", "gpred-window-f32", ("gsum", "parts")),
    ("gpred_at_free", "gpred-f32", ("gnext",)),
    ("border_in_inference", "forecast-f32", ("state",)),
    ("border_in_inference", "forecast-window-bf16", ("state",)),
    ("no_border_at_free", "inter3-f32", ("state", "border")),
    ("no_border_at_free", "inter2-bf16", ("border",)),
    ("window_shift", "window-wrap-f32", ("x",)),
    ("window_shift", "window-bf16", ("x",)),
    ("swap_statics_forcing", "feed-f32", ("x",)),
    ("mask_inverted", "nan-f32", ("x",)),
    ("weight_at_free", "inter3-f32", ("dy", "loss")),
    ("weight_at_free", "inter2-bf16", ("dy", "loss")),
    ("dx_at_call0", "feed-f32", ("sentinel",)),          # a written buffer, through the comparison the recorder makes
    # the model call between its two ends: nothing but the block nodes looks there
    ("eval_batch_stats", "eval-bf16", ("norm",)),
    ("eval_batch_stats", "eval20-bf16", ("norm",)),
    ("mid_block_weights", "eval-bf16", ("Ymid",)),
    ("mid_block_weights", "forecast-f32", ("Ymid",)),
    ("mid_block_weights", "feed-bf16", ("Ymid",)),
    # the model's backward on another call's saved workspace: the data gradient and the parameter gradients are the detectors
    ("saved_of_next_call", "feed-f32", ("dx", "pgrad")),
    ("saved_of_next_call", "window-wrap-f32", ("dx", "pgrad")),
    ("lgrad_row_swapped", "feed-bf16", ("lgrad",)),
]


def test_every_wrong_wiring_is_planted_somewhere():
    assert {w for w, _, _ in SENSITIVITY} == set(RN.WRONG)


@pytest.mark.parametrize("wrong,name,detectors", SENSITIVITY, ids=[f"{w}-{n}" for w, n, _ in SENSITIVITY])
def test_wrong_wiring_moves_its_detector_by_ten_bars(wrong, name, detectors):
    case, c, ref, run = _chain(name, wrong)
    fig = RN.check(run, ref)
    bars = RN.bars_of(case)
    for node in detectors:
        moved = RN.node_value(fig, node)
        bar = bars[node]
        bar = max(bar) if isinstance(bar, tuple) else bar
        print(f"{wrong} in {name}: {node} moves by {moved:.3e} (bar {bar:.1e})")
        assert moved > 0 and moved >= 10 * bar, f"{wrong} in {name}: {node} moves by {moved:.3e}, its bar is {bar:.1e}"


def test_fused_tail_composite_sees_a_forced_border_in_a_forecast():
    """bf16 flavour: y is never stored, the composite "new state - prev" is the detector of the state update.  With the y records
    withheld, as on the device, a forecast that forces its border moves the composite by 10 x its bar."""
    case, c, ref, run = _chain("forecast-window-bf16", "border_in_inference")
    for rec in run.calls:
        rec["y"] = None
    moved = RN.node_value(RN.check(run, ref), "inc")
    bar = max(RN.BARS_BF16["inc"])
    print(f"border_in_inference, y withheld: inc moves by {moved:.3e} (bar {bar:.1e})")
    assert moved >= 10 * bar
