"""
The native HalfUNet rollout (py4cast_amd/halfunet_rollout.py) call by call against float64: each case of the table
(tests/rollout_nodes.py::CASES) runs ONCE through AutoRegressiveLightning under the recorder -- training_step + backward(), a validation
step on the .eval() model, or the forecast of phase "inference" -- and every node of the T * K calls is checked ALONE from the values
the device stored upstream of it (tests/rollout_nodes.py::check), with the call, the quantity and the case in the message.  What the
checker can see is proven on the CPU first (tests/test_rollout_nodes_cpu.py: every wrong wiring moves its detector by >= 10 bars).

Forward, per call c = (i, k): the network input x_c (window order, statics, forcing[:, i] -- again at a free step --, mask channel, zero
padding; the next input a fused step emitted is what call c + 1 read), the previous state read, the slot written; the model call
block by block -- Y[0] = conv(x_c) (the call read this x), Y[1] .. Y[11] each the convolution, with this model's weights, of the
input formed from the stored maps upstream of it (activation, max-pool, the sum of the up-sampled levels), the normalisation arrays
of every block from the statistics of its stored Y[j] (from the running statistics in eval), y_c = 1x1 convolution of the stored
decoder output --; the new state from stored prev and stored y (two-kernel route, bit-equal) or "new state - prev" from the stored
decoder output (fused tail: y is never written), the border points, loss[:, i], pred[:, i], fused_loss, the mask count, the
running statistics after T * K calls (torch's rule on the statistics of every call's stored Y[i]).  Backward, per call: what
arrives at the new state (g_next = dprev of call c + 1 (+ g_pred[:, i] at a loss step), the rows of dx_{c+1}; windowed sweep: the
part list of p4c_sum_state_grads by the buffer each part points at, then gsum), the saved loss gradient lgrads[i] against the
float64 gradient at the stored new state and target, dy_c and dprev_c by autograd through the float64 step, dx_c and, summed over
the calls (also into pre-filled gradients under FlatDDP), every p.grad; dprev and dx of call 0 keep their sentinel, the padded
input channels of dx and the channels of dy beyond F are zero.

The model-call nodes take every decision from the call's stored maps.  Re-run from x alone, a model call meets the device only
while both take every ReLU and max-pool decision alike, and on this grid (coarsest level 2 x 3) one decision of the 8 x 12 ..
2 x 3 levels moves a gradient by 1e-2 .. 1e-1.  Measured that way, fp32: dx up to 6.2e-2 and p.grad up to 4.3e-2
(window-wrap-f32; inter3-f32 3.4e-2 / 1.0e-2, gpred-f32 1.2e-2 / 9.6e-3, gpred-window-f32 8.5e-3 / 7.2e-3, diff-f32 5.3e-3 on a
p.grad; 2e-5 elsewhere) against the 5e-3 of tests/test_model_gpu.py.  bf16 storage: y 3.7e-2 per element / 3.3e-2 in the 2-norm,
dx 0.45 / 0.44, p.grad up to 0.48 -- and the float64 reference with its own maps and weights rounded to bf16 shows 3.4e-2 /
2.9e-2, 0.44 / 0.42 and 0.48 against itself unrounded: the storage format's figures, which permit no bar below the 5e-2 of
tests/test_wide_rollout_gpu.py.  So the recorder keeps each call's ``saved`` workspace and the references work from the raw
convolution outputs Y[i] and the normalisation arrays in it (tests/rollout_nodes.py::stored_forward / stored_backward, on the
node references of tests/halfunet_nodes.py), as tests/test_halfunet_nodes_gpu.py does inside one call ("Where a gradient buffer
ends up holding dY").  Nothing of the stored forward is taken on trust: every Y[j] and every normalisation array is itself a
node, so the model call is asserted from x to y in both flavours, one block at a time.  The whole call re-run from x alone stays
asserted on top of that for fp32 (y 1e-4, running statistics 1e-4) and is printed for bf16.

Cases at F = 12 / Fs = 4 / Ff = 5 with one input state: the 16-byte step cannot emit the next input there (5 tail quads, 4 lanes per grid
point) and the bf16 flavour keeps the two-kernel route (the flat kernel takes the 1x1 convolution only off the 16-byte grid); feed-f32
runs the flat step with the next input, feed-bf16 / inter2-bf16 / eval-bf16 store y in bf16 and save the loss gradients.  The cases at
F = 20 (feed20-f32, feed20-bf16, inter2-20-bf16, eval20-bf16) reach what those rows were after: the 16-byte step emitting the next
input, and the fused tail together with "feed next step".  Every case asserts its route (assert_route).

Bars (worst measured on one MI355X / bar, where it was met: profiles/rollout_nodes.txt has every case):
  bit-equal: x, emitted next input, prev, slot, new state (fp32 torch chain), border, pred, fused_loss, count, g_next, the rows of
      dx_{c+1}, parts, gsum, sentinels, zero channels          tests/test_loop_trips_gpu.py (element outputs, p4c_sum_state_grads)
  loss                    1.6e-7 / 1e-5                          tests/test_loop_trips_gpu.py (reductions)
  dy                      fp32 0 / 1e-5 with the 4-ulp floor; bf16 rows 3.9e-3 / 2^-8 (one bf16 rounding)   tests/test_loop_trips_gpu.py
  dprev                   0 / 1e-5 with the 4-ulp floor          tests/test_loop_trips_gpu.py
  running statistics      3.2e-7 (fp32), 2.1e-7 (bf16) / rtol 1e-4, atol 1e-5       tests/test_model_gpu.py
  y from x (fp32)         6.6e-6 / 1e-4 per element              tests/test_model_gpu.py
  Y[0], y, new state - prev   fp32 3.5e-7 / 1e-5 (2-norm); bf16 3.5e-3 / 6e-3 per element, 1.7e-3 / 3e-3 2-norm
                                                                 tests/test_halfunet_nodes_gpu.py (forward maps)
  Y[1] .. Y[11]           fp32 4.3e-7 / 1e-5 (Y[10], diff-f32 call 1); bf16 3.7e-3 / 6e-3 per element (Y[9], inter2-bf16 call 4),
                          1.8e-3 / 3e-3 2-norm (Y[9], inter2-20-bf16 call 2)     tests/test_halfunet_nodes_gpu.py (forward maps)
  normalisation arrays    fp32 2.8e-7 / 9e-7 (norm[2].shift, feed20-f32 call 0); bf16 9.3e-8 / 4e-7 (norm[2].shift, inter2-20-bf16
                          call 2)                                tests/test_halfunet_nodes_gpu.py (norm arrays, per storage type)
  saved loss gradients    3.9e-3 / 2^-8 (one bf16 rounding)      tests/test_loop_trips_gpu.py (saved loss gradient)
  dx, p.grad (fp32)       2.2e-6, 1.9e-6 / 5e-3                  the floor of _noise_bar at T = 1 in tests/test_model_gpu.py::
                                                                 test_training_step_with_halfunet_matches_oracle (the 10 x err32 term is
                                                                 not used: the bar asks more than the bar that test sets)
  dx (bf16)               1.04e-2 per element, 9.0e-3 2-norm (feed-bf16, call 2) / 4e-2      4 x measured = 4.2e-2 and 3.6e-2
  p.grad (bf16)           1.19e-2 (flat-bf16, encoder1.enc1norm2.bias) / 4e-2                4 x measured = 4.8e-2
      (no precedent: twelve blocks chained from the stored forward, where the plan test checks one block from stored gradients; held
      at 4e-2, under the 5e-2 the native-versus-generic tests allow.  dx and p.grad are the detectors of one wiring of the CPU file,
      the backward handed another call's saved workspace, which is planted in fp32 cases against the 5e-3 bar)
The whole file takes about 9 s on one MI355X (device 1.2 s, float64 references on the CPU 5 s), next to the "about 6 s" of the
plan test.
"""
import os
import sys
import time
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rollout_nodes as RN  # noqa: E402

pytestmark = pytest.mark.gpu

FORWARD = {"x", "xnext", "prev", "slot", "state", "inc", "border", "Y0", "Ymid", "norm", "ytail", "y_x", "loss", "pred", "fused_loss", "count"}
STATS = {"running", "running_x", "nbt", "running_untouched"}
BACKWARD = {"gnext", "gnext2", "parts", "gsum", "lgrad", "dy", "dyzero", "dprev", "sentinel", "dx", "dxzero"}
PGRAD = {"pgrad"}


class Run(SimpleNamespace):
    def __repr__(self):
        return f"Run({self.name})"


def _entries(run, which):
    recs = run.calls if which == "fwd" else [run.bwd[c] for c in sorted(run.bwd)]
    return [[e for e in r["entries"]] for r in recs]


def _count(run, which, name):
    return sum(e.count(name) for e in _entries(run, which))


def assert_route(name, run, lm):
    """the case reached what its row of the table names: the library's own predicates and the recorded entry points"""
    from py4cast_amd import halfunet_rollout as HR

    case = RN.CASES[name]
    T, K, T_in, F = case.T, case.K, case.T_in, case.F
    ncalls = T * K
    feed, v4_next, flat_next = HR._step_paths(lm.model, T_in, RN.N, F, case.Fs, int(case.nan))
    fused_tail = HR._fused_tail(lm.model, v4_next, flat_next, F, int(case.nan))
    assert len(run.calls) == ncalls and _count(run, "fwd", "p4c_halfunet_forward") == ncalls, f"{name}: {len(run.calls)} native calls"
    assert _count(run, "fwd", "p4c_ar_update_fwd") == 0, f"{name}: the generic update ran"
    assert feed == (T_in == 1) == run.feed and fused_tail == run.fused_tail, (name, feed, fused_tail)
    assert (lm.model.act_dtype == torch.bfloat16) == case.bf16
    fused_step = feed and (v4_next or flat_next)
    assert run.fuse_next == fused_step
    builds = _count(run, "fwd", "p4c_build_x")
    emitted = sum(r["x_next"] is not None for r in run.calls)
    assert builds == (1 if fused_step else ncalls) and emitted == (ncalls - 1 if fused_step else 0), (name, builds, emitted)
    free = ("p4c_out_conv_update_fwd" if fused_tail else "p4c_ar_update_next")
    nfree = ncalls if case.mode == "forecast" else T * (K - 1)
    assert _count(run, "fwd", free) == nfree and sum(r["free"] for r in run.calls) == nfree, (name, nfree)
    if case.mode == "train":
        assert run.finished and sorted(run.bwd) == list(range(ncalls)) and _count(run, "bwd", "p4c_halfunet_backward") == ncalls
        assert run.save_lg == (case.bf16 and not case.nan) == (run.lgrads is not None), f"{name}: saved loss gradients"
        assert _count(run, "bwd", "p4c_ar_update_loss_bwd_saved" if run.save_lg else "p4c_ar_update_loss_bwd") == T
        assert _count(run, "bwd", "p4c_ar_update_next_bwd") == T * (K - 1)
        assert run.sweep == ("_sweep_window" if T_in > 1 else "_sweep")
        assert len({r["saved_ptr"] for r in run.calls}) == ncalls, f"{name}: one saved buffer per call"
    else:
        assert not run.bwd and len({r["saved_ptr"] for r in run.calls}) == 1, f"{name}: one saved buffer for all calls"
    loss_entry = "p4c_out_conv_update_loss_fwd" if fused_tail else None
    assert all((r["y"] is None) == fused_tail for r in run.calls), f"{name}: y is stored on the two-kernel route only"
    if name in ("feed-f32", "feed20-f32"):
        assert fused_step and v4_next == (name == "feed20-f32"), f"{name}: the 16-byte step emits the next input at F = 20 only"
        assert _count(run, "fwd", "p4c_ar_update_loss_fwd_next") == T - 1 and _count(run, "fwd", "p4c_ar_update_loss_fwd") == 1
    elif name == "feed-bf16":
        assert fused_step and not v4_next and flat_next     # two-kernel route with the saved loss gradients (see the table)
        assert _count(run, "fwd", "p4c_ar_update_loss_fwd_next_saved") == T
    elif name in ("feed20-bf16", "flat-bf16"):
        assert fused_step and _count(run, "fwd", loss_entry) == T
        assert (v4_next, F % 4) == ((False, 1) if name == "flat-bf16" else (True, 0)) and flat_next
    elif name == "inter3-f32":
        assert {r["slot"] for r in run.calls} == {("inter", 0), ("inter", 1), ("pred", 0), ("pred", 1)}, "both scratch buffers, re-used"
        assert _count(run, "fwd", "p4c_ar_update_loss_fwd_next") + _count(run, "fwd", "p4c_ar_update_loss_fwd") == T
    elif name in ("inter2-bf16", "inter2-20-bf16"):
        assert [r["step"] for r in run.calls] == ["_free_step", "_loss_step"] * T
        assert _count(run, "fwd", loss_entry or "p4c_ar_update_loss_fwd_next_saved") == T
    elif name in ("window-wrap-f32", "window-bf16", "gpred-window-f32"):
        bufs = [run.bwd[c]["dx_ptr"] for c in range(1, T)]
        assert T - 1 >= T_in + 1, "the ring index k % (T_in + 1) wraps"
        assert len(set(bufs)) <= T_in + 1
        if name == "window-wrap-f32":
            assert len(set(bufs)) == T_in + 1 < len(bufs), f"{name}: a buffer of the ring is written twice ({len(set(bufs))} buffers, {len(bufs)} dx)"
        if name == "window-bf16":
            assert run.dxc == T_in * F > RN.NF and run.bwd[1]["dx"].shape[-1] == 2 * RN.NF, "state channels cross the 64-channel block"
            assert _count(run, "fwd", loss_entry) == T
        assert _count(run, "bwd", "p4c_sum_state_grads") == (T if name == "gpred-window-f32" else T - 1)
    elif name == "window-short-f32":
        assert T < T_in + 1 and len({run.bwd[c]["dx_ptr"] for c in range(1, T)}) == T - 1
    elif name == "nan-f32":
        assert builds == ncalls and run.count > 0 and not run.save_lg and lm.model.in_channels == case.cin
    elif name == "diff-f32":
        assert run.ops.std is None and run.ops.mean is None
    if case.gpred:
        assert run.ops.g_pred is not None, f"{name}: no gradient arrived at the prediction"
    elif case.mode == "train":
        assert run.ops.g_pred is None
    if case.mode == "eval":
        assert not run.training
    if case.mode == "forecast":
        assert run.training and run.loss is None and len({r["x_ptr"] for r in run.calls}) == (2 if fused_step else 1), "the x ring"


def _figures(name, device):
    case = RN.CASES[name]
    t0 = time.time()
    run, lm, rec, c = RN.device_run(name, device)
    t1 = time.time()
    ref64 = RN.make_ref(case, run.state0)
    fig = RN.check(run, ref64)
    print(f"\n[rollout-nodes] {name}: device {t1 - t0:.2f} s, references {time.time() - t1:.2f} s")
    return Run(name=name, case=case, run=run, lm=lm, c=c, fig=fig)


@pytest.fixture(scope="module", params=list(RN.CASES))
def run(request, gpu_device):
    r = _figures(request.param, gpu_device)
    yield r
    del r.lm, r.run, r.fig
    torch.cuda.empty_cache()


def _check(run, nodes):
    """prints worst value / bar per node before it asserts"""
    fig = [f for f in run.fig if f[0] in nodes]
    failures, worst = RN.judge(run.case, fig)
    print(f"\n[rollout-nodes] {run.name}: " + "; ".join(f"{k} {v:.2e} / {lim:.0e} [{what}]" for k, (v, lim, what) in sorted(worst.items())))
    assert not failures, f"{run.name}:\n" + "\n".join(failures)
    return {f[0] for f in fig}


def test_route(run):
    assert_route(run.name, run.run, run.lm)


def test_operands_are_the_batch(run):
    """what the rollout handed to its kernels is the batch and the module's statistics, element for element"""
    case, ops = run.case, run.run.ops
    want = RN.operands_of(case, run.c, torch.float32)
    for n in ("inputs", "forcing", "outputs", "statics", "std", "mean", "border", "interior"):
        a, b = getattr(ops, n), getattr(want, n)
        if n in ("border", "interior") and (case.mode == "forecast" or (n == "border" and case.strategy != "scaled_ar")):
            continue      # (a forecast forces no border and has no loss: it is handed neither mask)
        assert (a is None) == (b is None), n
        if a is not None:
            assert RN.unequal(a.contiguous(), b.contiguous()) == 0.0, f"{run.name}: operand {n}"
    if case.mode != "forecast":
        assert RN.rel2(ops.weights, RN.operands_of(case, run.c, torch.float64).weights) < 1e-6
        assert ops.num_interior == want.num_interior and ops.kind == "mse"
    if case.mode == "train":
        assert RN.unequal(ops.gl, want.gl) == 0.0, "the gradient of the loss rows is weight / (B T)"


def test_forward_nodes(run):
    seen = _check(run, FORWARD)
    assert {"x", "prev", "slot", "pred", "Y0", "Ymid", "norm"} <= seen and ("inc" if run.run.fused_tail else "state") in seen


def test_running_statistics(run):
    seen = _check(run, STATS)
    assert "nbt" in seen and ("running" if run.case.mode != "eval" else "running_untouched") in seen


def test_backward_nodes(run):
    seen = _check(run, BACKWARD)
    if run.case.mode != "train":
        assert not seen and not run.run.bwd      # nothing was differentiated
        return
    assert {"dy", "sentinel", "gnext2"} <= seen and ("gsum" if run.case.T_in > 1 else "gnext") in seen
    assert ("lgrad" in seen) == run.run.save_lg
    assert ("dx" in seen) == (run.case.T * run.case.K > 1)


def test_parameter_gradients(run):
    seen = _check(run, PGRAD)
    assert ("pgrad" in seen) == (run.case.mode == "train")


@pytest.mark.parametrize("name", ["window-wrap-f32"])
def test_sweep_adds_into_prefilled_gradients(gpu_device, name):
    """parameter gradients pre-filled through FlatDDP(m, 1): the sweep ADDS -- p.grad - prefill is the sum of the calls' float64
    gradients on the stored operands, at the bar of the parameter gradients"""
    from py4cast_amd.trainer import FlatDDP

    plain, lm, _, _ = RN.device_run(name, gpu_device)
    prefill, keep = {}, {}

    def before(lm):
        keep["ddp"] = FlatDDP(lm, 1)
        assert lm.model._flat_grad_target() is not None
        g = torch.Generator(device=gpu_device).manual_seed(11)
        for n, p in lm.model.named_parameters():
            scale = float(plain.pgrads[n].abs().max())
            prefill[n] = scale * (torch.rand(p.shape, device=p.device, generator=g) + 0.5) * (
                1 - 2 * (torch.rand(p.shape, device=p.device, generator=g) < 0.5).float())
            p.grad.copy_(prefill[n])

    run, lm, _, _ = RN.device_run(name, gpu_device, before=before)
    assert float(keep["ddp"].flat_grad.abs().sum()) > 0
    for n in run.pgrads:
        run.pgrads[n] = run.pgrads[n] - prefill[n].cpu()
    # (the subtraction costs up to 2^-24 of the prefill, which is of the gradient's own size: far below the bar)
    ref64 = RN.make_ref(RN.CASES[name], run.state0)
    fig = [f for f in RN.check(run, ref64) if f[0] == "pgrad"]
    assert len(fig) == len(run.pgrads)
    _check(Run(name=name + " (prefilled)", case=RN.CASES[name], fig=fig), PGRAD)
