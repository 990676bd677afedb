"""
TEST INFRASTRUCTURE ONLY.  The native HalfUNet rollout (py4cast_amd/halfunet_rollout.py) call by call: the table of cases, float64
references of every native call, a reference chain that composes them over a schedule, a recorder of what the device's calls wrote,
and ONE checker (``check``) that judges a set of records -- the device's (tests/test_rollout_nodes_gpu.py) or the reference chain's
with a wrong wiring planted (tests/test_rollout_nodes_cpu.py) -- node by node, each node from the STORED values upstream of it.

Layout: everything is flat, states (B, N, F), network rows (B, N, C), masks (N,), as tests/step_reference.py (whose element and
step references are used here: tests/test_step_reference_cpu.py proves them; tests/test_rollout_nodes_cpu.py proves their
composition against oracle/rollout.py + oracle/losses.py).  The references and the checker use no product code; only the recorder
and ``device_run`` do (``case_inputs`` takes the shared synthetic tensors of tests/helpers.py).  The model-call nodes work from the
maps each call stored, on the node references of tests/halfunet_nodes.py: see "the model call from its stored maps" below.
"""
import copy
import math
from dataclasses import dataclass
from types import SimpleNamespace

import torch

import halfunet_nodes as HN
import step_reference as R

B, H, W = 2, 32, 48      # the smallest grid with a non-square 2 x 3 coarsest level
N = H * W
NF = 64                  # channels of the network's output rows (y, dy) and of a block of dx
SENT = 7.0
EPS32 = 2.0 ** -23
BF16_RND = 2.0 ** -8
LOSS_WEIGHT = 0.7
GPRED = 0.3


@dataclass(frozen=True)
class Case:
    bf16: bool
    strategy: str
    T_in: int
    K: int
    T: int
    F: int
    Fs: int
    Ff: int
    border: int
    nan: bool = False
    gpred: bool = False
    mode: str = "train"      # train | eval (model.eval(), no_grad) | forecast (phase "inference")
    seed: int = 9

    @property
    def cin(self):
        return self.T_in * self.F + self.Fs + self.Ff + int(self.nan)


CASES = {
    "feed-f32": Case(False, "scaled_ar", 1, 1, 3, 12, 4, 5, 2),
    "feed-bf16": Case(True, "scaled_ar", 1, 1, 3, 12, 4, 5, 2),
    "flat-bf16": Case(True, "scaled_ar", 1, 1, 3, 21, 4, 21, 2),
    "inter3-f32": Case(False, "scaled_ar", 1, 3, 2, 12, 4, 5, 2),
    "inter2-bf16": Case(True, "scaled_ar", 1, 2, 3, 12, 4, 5, 2),
    "window-wrap-f32": Case(False, "scaled_ar", 2, 1, 5, 12, 4, 5, 2),
    "window-short-f32": Case(False, "scaled_ar", 3, 1, 2, 12, 4, 5, 2),
    "window-bf16": Case(True, "scaled_ar", 2, 1, 4, 40, 4, 5, 2),
    "nan-f32": Case(False, "scaled_ar", 1, 1, 3, 12, 4, 5, 0, nan=True),
    "diff-f32": Case(False, "diff_ar", 1, 1, 3, 12, 4, 5, 0),
    "gpred-f32": Case(False, "scaled_ar", 1, 2, 2, 12, 4, 5, 2, gpred=True),
    "gpred-window-f32": Case(False, "scaled_ar", 2, 1, 4, 12, 4, 5, 2, gpred=True),
    "eval-bf16": Case(True, "scaled_ar", 1, 1, 2, 12, 4, 5, 2, mode="eval"),
    "forecast-f32": Case(False, "scaled_ar", 1, 2, 3, 12, 4, 5, 2, mode="forecast"),
    "forecast-window-bf16": Case(True, "scaled_ar", 2, 1, 3, 12, 4, 5, 2, mode="forecast"),
    # One input state at F = 12 / Fs = 4 / Ff = 5 (32 padded input channels): the 16-byte step cannot emit the next input (5 tail quads
    # over 4 lanes per grid point), the flat step serves, and the bf16 flavour keeps the two-kernel route there (the flat kernel takes
    # the 1x1 convolution as its front end only off the 16-byte grid).  F = 20 is the smallest feature count at which one input state
    # reaches the 16-byte step with the next input and, in bf16, the fused tail together with "feed next step".
    "feed20-f32": Case(False, "scaled_ar", 1, 1, 3, 20, 4, 5, 2),
    "feed20-bf16": Case(True, "scaled_ar", 1, 1, 3, 20, 4, 5, 2),
    "inter2-20-bf16": Case(True, "scaled_ar", 1, 2, 3, 20, 4, 5, 2),
    "eval20-bf16": Case(True, "scaled_ar", 1, 1, 2, 20, 4, 5, 2, mode="eval"),
}

# node -> bar.  0.0: bit-equal.  A pair is (per element of the largest magnitude, relative 2-norm).  Where each bar comes from: the
# docstring of tests/test_rollout_nodes_gpu.py.  The model call is asserted block by block from the stored maps in both flavours
# (Y0, Ymid, norm, ytail / inc); "y_x" / "running_x" (the whole call and the running statistics re-run from x alone) are asserted on
# top of that for the fp32 flavour and only printed for bf16 (inf): see "the model call from its stored maps".
_EQUAL = {k: 0.0 for k in ("x", "xnext", "prev", "slot", "state", "border", "pred", "fused_loss", "count", "nbt", "gnext", "gnext2",
                           "parts", "gsum", "sentinel", "dxzero", "dyzero", "running_untouched")}
_MAP = (6e-3, 3e-3)      # a bf16-stored map against float64 (tests/test_halfunet_nodes_gpu.py, tests/test_unet_nodes_gpu.py)
# norm: the normalisation arrays of tests/test_halfunet_nodes_gpu.py, per storage type.
# fp32 dx / pgrad: the floor of tests/test_model_gpu.py::_noise_bar at T = 1, per element of the largest magnitude.  bf16 dx / pgrad
# (2-norm for pgrad): measured 1.04e-2 / 9.0e-3 and 1.19e-2 on one MI355X; 4 x that is 4.2e-2 / 3.6e-2 and 4.8e-2, held at 4e-2.
BARS_F32 = dict(_EQUAL, Y0=1e-5, Ymid=1e-5, norm=9e-7, ytail=1e-5, y_x=1e-4, loss=1e-5, running=1e-4, running_x=1e-4, dy=1e-5, dprev=1e-5,
                dx=5e-3, pgrad=5e-3)
BARS_BF16 = dict(_EQUAL, Y0=_MAP, Ymid=_MAP, norm=4e-7, ytail=_MAP, inc=_MAP, y_x=(math.inf, math.inf), loss=1e-5, running=1e-4,
                 running_x=math.inf, lgrad=BF16_RND, dy=BF16_RND, dprev=1e-5, dx=(4e-2, 4e-2), pgrad=4e-2)


def bars_of(case):
    return BARS_BF16 if case.bf16 else BARS_F32


# ------------------------------------------------------------------------------------------------ inputs
def case_inputs(case):
    """helpers.synthetic_case (grid layout) with the NaNs of tests/test_inter_steps_rollout_gpu.py::_case planted for any T"""
    from helpers import synthetic_case

    c = synthetic_case(seed=case.seed, B=B, T=case.T, T_in=case.T_in, H=H, W=W, F=case.F, Ff=case.Ff, Fs=case.Fs, border=case.border)
    if case.nan:
        c["inputs"][0, 0, 3, 4, 1] = float("nan")
        c["forcing"][-1, -1, 5, 6, 2] = float("nan")
        c["outputs"][:, :, 7, 8, :] = float("nan")
        c["outputs"][0, -1, 2, 2, 0] = float("nan")
    return c


def flat(t):
    """(..., H, W, C) -> (..., N, C)"""
    return t.reshape(*t.shape[:-3], t.shape[-3] * t.shape[-2], t.shape[-1])


def operands_of(case, c, dtype):
    """The rollout's operands in the flat layout, as the reference derives them from the case (test_model_gpu.py::run_ref)."""
    from oracle.losses import weighted_loss_weights

    forecast = case.mode == "forecast"
    scaled = case.strategy == "scaled_ar"
    interior = (1.0 - c["border_mask"]).to(dtype)
    ops = SimpleNamespace(
        inputs=flat(c["inputs"]).to(dtype), forcing=flat(c["forcing"]).to(dtype),
        outputs=None if forecast else flat(c["outputs"]).to(dtype),
        statics=flat(c["statics"]).to(dtype).unsqueeze(0).expand(B, N, case.Fs),
        std=c["diff_std"].to(dtype) if scaled else None, mean=c["diff_mean"].to(dtype) if scaled else None,
        border=c["border_mask"].to(dtype).reshape(N), interior=interior.reshape(N),
        weights=weighted_loss_weights(c["state_weight"].to(dtype), c["diff_std"].to(dtype), "mse"),
        num_interior=float(interior.sum()), count=0, kind="mse", gl=None, g_pred=None)
    if not forecast:
        ops.count = R.masked_count(ops.outputs, "from_nan" if case.nan else "none")
        ops.gl = torch.full((B, case.T), LOSS_WEIGHT / (B * case.T), dtype=dtype)
    return ops


def gpred_weights(case):
    """R of the cases that differentiate through the prediction itself: loss + GPRED * (pred * R).sum()"""
    g = torch.Generator().manual_seed(case.seed + 100)
    return torch.randn(B, case.T, N, case.F, generator=g)


def make_ref(case, state_dict=None, seed=0):
    """oracle/halfunet.py::HalfUNetRef in float64 -- with the device model's state_dict, or seeded with non-trivial affine parameters
    (tests/test_model_gpu.py::_make_pair)"""
    from oracle.halfunet import HalfUNetRef

    torch.manual_seed(seed)
    ref = HalfUNetRef(case.cin, case.F)
    if state_dict is not None:
        ref.load_state_dict(state_dict)
    else:
        with torch.no_grad():
            for m in ref.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-0.3, 0.3)
    return ref.double()


# ------------------------------------------------------------------------------------------------ references per call
def ref_input(window, statics, forcing_i, T_in, mask_on_nan, c_pad, dtype):
    """oracle.rollout.next_x on the window of states (B, T_in, N, F) + zero padding to c_pad channels + the cast to the rows' type"""
    from oracle.rollout import next_x

    x = next_x(window, statics, forcing_i, T_in, mask_on_nan).to(window.dtype)
    if c_pad is not None and c_pad > x.shape[-1]:
        x = torch.cat([x, x.new_zeros(*x.shape[:-1], c_pad - x.shape[-1])], dim=-1)
    return x.to(dtype)


def ref_update(prev, y, std, mean, border_state, border, interior, strategy, free, inference, mask_on_nan, dtype=torch.float64):
    """oracle/rollout.py:126-141 for one call: last_prev (+ y * std + mean when scaled), border forcing in training and validation
    -- at a free (intermediary) step too, never in inference.  In the kernels' operation order, so dtype=float32 is the fp32 torch
    chain the device equals bit for bit."""
    scaled = strategy == "scaled_ar"
    forced = scaled and not inference
    return R.ar_update(prev, y, border_state if forced else None, std if scaled else None, mean if scaled else None,
                       border if forced else None, interior if forced else None, 1.0, mask_on_nan, dtype)


def ref_loss(new, target, weights, interior, num_interior, count, kind, mask):
    """the weighted loss of row (b, i) in float64 -> (B,): oracle/losses.py::weighted_loss for one time step"""
    m, t = R.resolve_mask(target, "from_nan" if mask else "none")
    e = R._elem(new.double(), t, m, kind)
    return ((e * weights.double()).sum(-1) * interior.double()).sum(-1) / (num_interior - count)


def ref_step_adjoint(prev, y, new_stored, target, ops, case, free, gl_i, g_next, g_next2, lgrad=None, ycs=NF, loss_at_free=False):
    """(dy (B, N, ycs), dprev (B, N, F)) of one AR step by autograd through the float64 ref_update + ref_loss: the objective is
    sum(gl_i * loss) (loss steps) + sum((g_next + g_next2[..., :F]) * new).  ``new_stored``: the loss is evaluated at the state the
    device stored (straight-through); ``lgrad``: from the saved loss gradients instead, linear in the state."""
    F = prev.shape[-1]
    p64 = prev.double().requires_grad_(True)
    y64 = (torch.zeros(*prev.shape[:-1], ycs, dtype=torch.float64) if y is None else y.double()).requires_grad_(True)
    inference = case.mode == "forecast"
    new = ref_update(p64, y64, ops.std, ops.mean, target, ops.border, ops.interior, case.strategy, free, inference, case.nan)
    ns = new if new_stored is None else new + (new_stored.double() - new).detach()
    obj = ns.new_zeros(())
    if (not free) or loss_at_free:
        if lgrad is not None:
            coef = (gl_i.double() / (ops.num_interior - ops.count))[:, None, None] * ops.interior.double()[None, :, None] * ops.weights.double()
            obj = obj + (coef * lgrad.double() * ns).sum()
        else:
            obj = obj + (gl_i.double() * ref_loss(ns, target, ops.weights, ops.interior, ops.num_interior, ops.count, ops.kind, case.nan)).sum()
    if g_next is not None:
        obj = obj + (g_next.double() * ns).sum()
    if g_next2 is not None:
        obj = obj + (g_next2[..., :F].double() * ns).sum()
    dy, dprev = torch.autograd.grad(obj, [y64, p64], allow_unused=True)
    return (torch.zeros_like(y64) if dy is None else dy), (torch.zeros_like(p64) if dprev is None else dprev)


def ref_state_grad_sum(parts, F, dtype=torch.float64):
    """the windowed sum: parts = [(rows (B, N, C), channel offset)], summed left to right in ``dtype`` (float32: the fp32 torch chain
    p4c_sum_state_grads equals bit for bit, tests/test_loop_trips_gpu.py::test_sum_state_grads)"""
    acc = None
    for rows, off in parts:
        v = rows[..., off:off + F].to(dtype)
        acc = v if acc is None else acc + v
    return acc


def ref_model_vjp(ref, x, dy, train, keep_stats=False):
    """One model call of ``ref`` (HalfUNetRef, any float type) on stored operands: x (B, N, >= cin) rows, dy (B, N, >= cout) rows or
    None -> y (B, N, cout), dx (B, N, cin) or None, {parameter name: gradient}.  The running statistics move (train) only with
    ``keep_stats``."""
    dt = next(ref.parameters()).dtype
    cin, cout = ref.encoder1[0].in_channels, ref.outconv.out_channels
    before = None if keep_stats else {k: v.clone() for k, v in ref.named_buffers()}
    ref.train(train)
    xr = x[..., :cin].to(dt).reshape(x.shape[0], H, W, cin).permute(0, 3, 1, 2).contiguous().requires_grad_(dy is not None)
    with torch.set_grad_enabled(dy is not None):
        y = ref(xr)
    dx, grads = None, {}
    if dy is not None:
        params = dict(ref.named_parameters())
        g = torch.autograd.grad(y, [xr] + list(params.values()), dy[..., :cout].to(dt).reshape(x.shape[0], H, W, cout).permute(0, 3, 1, 2))
        dx = g[0].permute(0, 2, 3, 1).reshape(x.shape[0], N, cin)
        grads = {n: gr for n, gr in zip(params, g[1:])}
    if before is not None:
        with torch.no_grad():
            for k, v in ref.named_buffers():
                v.copy_(before[k])
    return y.detach().permute(0, 2, 3, 1).reshape(x.shape[0], N, cout), dx, grads


# ------------------------------------------------------------------------------------------------ the model call from its stored maps
# A whole model call re-run from x alone meets the device only as far as the two agree on every ReLU and max-pool decision between x
# and y: on this grid (coarsest level 2 x 3) one decision of the 8 x 12 .. 2 x 3 levels that falls the other way moves a gradient by
# 1e-2 .. 1e-1, in fp32 as in bf16, and with bf16 storage the forward itself differs by 3e-2 (the float64 reference with its maps
# rounded to bf16 shows the same figures: see tests/test_rollout_nodes_gpu.py).  So the model-call nodes get the treatment of
# tests/test_halfunet_nodes_gpu.py: the recorder keeps the call's ``saved`` workspace, and the references below work from the raw
# convolution outputs Y[i] and the normalisation arrays the device stored, every decision taken from them.  The stored maps are not
# taken on trust: ``check`` compares every Y[i] with the convolution of the input formed from the maps upstream of it and every
# normalisation array with the statistics of its Y[i] (the running statistics in eval), so the call is covered from x to y.
def plan_params(state):
    """the parameters of a HalfUNetRef state_dict in the plan's order [w0, gamma0, beta0, ..., w11, gamma11, beta11, wout] + names"""
    names = [n for n in state if not any(n.endswith(s) for s in ("running_mean", "running_var", "num_batches_tracked"))]
    assert len(names) == 3 * HN.NCONV + 1 and names[-1] == "outconv.weight" and names[0].endswith("conv1.weight"), names
    return [state[n].detach().double() for n in names]


def plan_names(state):
    return [n for n in state if not any(n.endswith(s) for s in ("running_mean", "running_var", "num_batches_tracked"))]


def plan_running(state):
    """[(running_mean, running_var)] of the 12 blocks, in the plan's order"""
    means = [state[n].detach().double() for n in state if n.endswith("running_mean")]
    var = [state[n].detach().double() for n in state if n.endswith("running_var")]
    assert len(means) == len(var) == HN.NCONV
    return list(zip(means, var))


def stored_forward(rec, cin, spec, as_device):
    """the forward of one call as chain_backward wants it, from the maps the device stored: Y[i] and norm[i] as stored, the activations
    and every block's input formed from them (as the kernels form them: ``as_device``)"""
    Y = [y.detach().double() for y in rec["Y"]]
    norm = [tuple(a.detach().double() for a in nrm) for nrm in rec["norm"]]
    A = [HN.act(Y[i], norm[i][0], norm[i][1], as_device=as_device) for i in range(HN.NCONV)]
    inp = []
    for i in range(HN.NCONV):
        if i == 0:
            v = rec["x"][..., :cin].detach().double().reshape(B, H, W, cin)
        elif i == 10:
            v = sum(HN.upsample(A[2 * k + 1], 1 << k) for k in range(HN.NLEV))
        elif i % 2 == 0:
            v = HN.pool(A[i - 1])
        else:
            v = A[i - 1]
        inp.append(spec.q(v))
    return SimpleNamespace(Y=Y, norm=norm, A=A, inp=inp)


def stored_backward(fw, params, spec, dy, stored):
    """halfunet_nodes.chain_backward on the stored forward ``fw``, with every gradient map the plan stores on its way (dA of each
    block, the rotating dP, dS and the x passes of the up-sampling adjoints) rounded to the storage type as its producer rounded it
    (``stored``; tests/test_halfunet_nodes_gpu.py::_backward does the same per node).  -> dx (B, H, W, cin), the 37 parameter
    gradients in the plan's order."""
    w, gamma, beta, wout = HN.split_params(params)
    grads = [None] * (3 * HN.NCONV + 1)

    def block(i, dA):
        sc, sh, mean, rstd = fw.norm[i]
        dgamma, dbeta, _, _, dY = HN.norm_bwd(stored(dA), fw.Y[i], HN.preact(fw.Y[i], sc, sh) > 0, mean, rstd, gamma[i], spec)
        grads[3 * i], grads[3 * i + 1], grads[3 * i + 2] = HN.conv_dw(fw.inp[i], spec.q(dY)), dgamma, dbeta
        return HN.conv_dx(spec.q(dY), spec.q(w[i]))

    dy = dy.detach().double()
    grads[36] = HN.conv_dw(spec.q(fw.A[11]), dy, 1)
    G0 = stored(block(10, block(11, HN.conv_dx(dy, spec.q(wout)))))
    dP = None
    for k in range(HN.NLEV - 1, -1, -1):
        dA = HN.up_adj_y(stored(HN.up_adj_x(G0, 1 << k)) if k else G0, 1 << k)
        if dP is not None:
            dA = dA + HN.pool_route(fw.A[2 * k + 1], stored(dP))
        dP = block(2 * k, block(2 * k + 1, dA))
    return dP, grads


# ------------------------------------------------------------------------------------------------ the schedule, stated once more
def schedule(case):
    """[(c, i, k, free)] of the T * K calls (lightning.py:565-662): call (i, k) is free for k < K - 1 and in a forecast"""
    return [(i * case.K + k, i, k, k < case.K - 1 or case.mode == "forecast") for i in range(case.T) for k in range(case.K)]


def expected_parts(case, i, gpred):
    """what state slot s = i + T_in collects in the windowed sweep: [(kind, call, channel offset)]"""
    parts = []
    if gpred:
        parts.append(("gpred", i, 0))
    if i + 1 < case.T:
        parts.append(("dprev", i + 1, 0))
    s = i + case.T_in
    for k in range(i + 1, min(i + case.T_in, case.T - 1) + 1):
        parts.append(("dx", k, (s - k) * case.F))
    return parts


# ------------------------------------------------------------------------------------------------ the reference chain
WRONG = ("free_forcing_next", "inter_to_pred", "gsum_drop_block", "gsum_offset_plus", "gsum_offset_minus", "drop_dprev", "gpred_dropped",
         "gpred_at_free", "border_in_inference", "no_border_at_free", "window_shift", "swap_statics_forcing", "mask_inverted",
         "weight_at_free", "dx_at_call0", "eval_batch_stats", "mid_block_weights", "saved_of_next_call", "lgrad_row_swapped")


def untouched(buf):
    """a buffer a call must not write still holds the sentinel in every element (the recorder's comparison, and the chain's)"""
    return bool((buf == SENT).all())


def chain(case, c, ref, wrong=None, dtype=torch.float64):
    """The per-call references composed over the schedule, forward and reverse sweep, as records in the recorder's format.
    ``wrong``: one of WRONG, planted the way the device would show it."""
    assert wrong is None or wrong in WRONG, wrong
    ops = operands_of(case, c, dtype)
    T, K, T_in, F = case.T, case.K, case.T_in, case.F
    forecast, train = case.mode == "forecast", case.mode != "eval"
    cpad = 32 * math.ceil(case.cin / 32)
    if case.gpred:
        ops.g_pred = GPRED * gpred_weights(case).to(dtype)
    ref = copy.deepcopy(ref)
    state0 = copy.deepcopy(ref.state_dict())
    win = [ops.inputs[:, t] for t in range(T_in)]
    calls = []
    loss = None if forecast else torch.zeros(B, T, dtype=dtype)
    pred = [None] * T
    garbage = torch.full((B, N, F), SENT, dtype=dtype)
    for cc, i, k, free in schedule(case):
        fi = i
        if wrong == "free_forcing_next" and k > 0:
            fi = min(i + 1, T - 1)
        w_ = win
        if wrong == "window_shift" and T_in > 1 and cc > 0:
            w_ = win[1:] + win[:1]
        st, fo = ops.statics, ops.forcing[:, fi]
        x = ref_input(torch.stack(w_, 1), st, fo, T_in, case.nan, cpad, dtype)
        if wrong == "swap_statics_forcing":
            x = torch.cat([x[..., :T_in * F], x[..., T_in * F + case.Fs:T_in * F + case.Fs + case.Ff], x[..., T_in * F:T_in * F + case.Fs],
                           x[..., T_in * F + case.Fs + case.Ff:]], -1)
        if wrong == "mask_inverted" and case.nan:
            x[..., case.cin - 1] = 1.0 - x[..., case.cin - 1]
        pp = plan_params(ref.state_dict())
        if wrong == "mid_block_weights":
            pp[3 * 5] = pp[3 * 4]               # block 5 convolves with another block's (say stale) prepared weights
        fwc = HN.chain_forward(x[..., :case.cin].reshape(B, H, W, case.cin), pp,
                               HN.Spec(training=train or wrong == "eval_batch_stats"), running=plan_running(ref.state_dict()))
        y, _, _ = ref_model_vjp(ref, x, None, train, keep_stats=True)
        if wrong in ("mid_block_weights", "eval_batch_stats"):
            y = fwc.y.reshape(B, N, F)
        prev = win[-1]
        if wrong == "inter_to_pred" and k > 0:
            prev = garbage                      # the scratch slot the schedule reads was never written
        tgt = None if forecast else ops.outputs[:, i]
        if wrong == "border_in_inference" and forecast:
            new = ops.border[:, None] * torch.nan_to_num(prev) + ops.interior[:, None] * ref_update(
                prev, y, ops.std, ops.mean, None, None, None, case.strategy, free, True, case.nan, dtype)
        elif wrong == "no_border_at_free" and free:
            new = ref_update(prev, y, ops.std, ops.mean, tgt, ops.border, ops.interior, case.strategy, free, True, case.nan, dtype)
        else:
            new = ref_update(prev, y, ops.std, ops.mean, tgt, ops.border, ops.interior, case.strategy, free, forecast, case.nan, dtype)
        if not forecast and (not free or wrong == "weight_at_free"):
            loss[:, i] += ref_loss(new, tgt, ops.weights, ops.interior, ops.num_interior, ops.count, ops.kind, case.nan).to(dtype)
        slot = ("pred", i) if (k == K - 1 or wrong == "inter_to_pred") else ("inter", k % 2)
        calls.append(dict(c=cc, i=i, k=k, free=free, x=x, x_next=None, y=y.to(dtype), prev=prev, new=new, slot=slot, entries=[],
                          Y=fwc.Y, norm=fwc.norm))
        if k == K - 1:
            pred[i] = new
        win = win[1:] + [new]
    run = SimpleNamespace(case=case, ops=ops, calls=calls, bwd={}, pred=None if pred[0] is None else torch.stack(pred, 1), loss=loss,
                          fused_loss=None if loss is None else loss * LOSS_WEIGHT, lgrads=None, cpad=cpad, dxc=T_in * F if T_in > 1 else case.cin,
                          state_dtype=dtype, row_dtype=dtype, state0=state0, buffers={k_: v.clone() for k_, v in ref.named_buffers()},
                          pgrads=None, count=ops.count, fused_tail=False, training=train)
    if case.mode != "train":
        return run
    # ---- reverse sweep
    total = {}
    gp = ops.g_pred
    dprev = None
    dxs = {}
    dxw = NF * math.ceil(run.dxc / NF)
    if wrong == "lgrad_row_swapped":            # the saved loss gradients, every forward step's in the row of the step before it
        lg = [2.0 * (calls[i * K + K - 1]["new"] - ops.outputs[:, i]) for i in range(T)]
        run.lgrads = torch.stack(lg[1:] + lg[:1])
    for cc, i, k, free in reversed(schedule(case)):
        rec = calls[cc]
        b = dict(c=cc, i=i, free=free, g_next=None, g_next2=None, parts=None, dprev_untouched=True, dx0_untouched=True)
        last = cc == T * K - 1
        if T_in == 1:
            g_next = None if last or wrong == "drop_dprev" else dprev
            take = gp is not None and (k == K - 1 or wrong == "gpred_at_free")
            if wrong == "gpred_dropped" and i == 0:
                take = False
            if take:
                g_next = gp[:, i] if g_next is None else g_next + gp[:, i]
            g_next2 = None if last else dxs[cc + 1]
        else:
            parts = expected_parts(case, i, gp is not None)
            if wrong == "drop_dprev":
                parts = [p for p in parts if p[0] != "dprev"]
            if wrong == "gpred_dropped" and i == 0:
                parts = [p for p in parts if p[0] != "gpred"]
            ndx = [j for j, p in enumerate(parts) if p[0] == "dx"]
            if wrong == "gsum_drop_block" and ndx:
                parts.pop(ndx[-1])
            shift = {"gsum_offset_plus": F, "gsum_offset_minus": -F}.get(wrong, 0)
            b["parts"] = [(kind, kk, off + (shift if kind == "dx" else 0)) for kind, kk, off in parts]
            tensors = []
            for kind, kk, off in parts:
                if kind == "gpred":
                    tensors.append((gp[:, i], 0))
                elif kind == "dprev":
                    tensors.append((dprev, 0))
                else:
                    tensors.append((torch.roll(dxs[kk], -shift, -1) if shift else dxs[kk], off))
            g_next = ref_state_grad_sum(tensors, F, dtype) if tensors else None
            g_next2 = None
        b["g_next"], b["g_next2"] = g_next, g_next2
        dy, dp = ref_step_adjoint(rec["prev"], rec["y"], rec["new"], None if forecast else ops.outputs[:, i], ops, case, free,
                                  ops.gl[:, i], g_next, g_next2, lgrad=None if (run.lgrads is None or free) else run.lgrads[i], ycs=NF,
                                  loss_at_free=wrong == "weight_at_free")
        b["dy"], b["dprev"] = dy.to(dtype), (dp.to(dtype) if cc > 0 else None)
        dprev = b["dprev"]
        # (saved_of_next_call: the model's backward handed the saved workspace of call cc + 1 -- it differentiates that call's forward)
        src = calls[cc + 1] if (wrong == "saved_of_next_call" and not last) else rec
        _, dx, grads = ref_model_vjp(ref, src["x"], dy, train)
        for n, g in grads.items():
            total[n] = g if n not in total else total[n] + g
        b["dx"] = None
        dxrows = torch.cat([dx[..., :run.dxc], dx.new_zeros(B, N, dxw - run.dxc)], -1).to(dtype)
        if cc > 0:
            b["dx"] = dxrows
            dxs[cc] = b["dx"]
        else:
            buf = torch.full_like(dxrows, SENT)     # call 0 is given no buffer to write: the recorder's sentinel, judged as it judges it
            if wrong == "dx_at_call0":
                buf.copy_(dxrows)
            b["dx0_untouched"] = untouched(buf)
        run.bwd[cc] = b
    run.pgrads = total
    return run


# ------------------------------------------------------------------------------------------------ the checker
def _d(t):
    return t.detach().double()


def rel2(got, ref):
    return float((_d(got) - _d(ref)).norm() / _d(ref).norm().clamp_min(1e-300))


def relmax(got, ref):
    return float((_d(got) - _d(ref)).abs().max() / _d(ref).abs().max().clamp_min(1e-300))


def unequal(got, ref):
    """0.0 where the two agree in every element (NaNs in the same places), otherwise the largest difference relative to the largest
    magnitude (inf where shapes, types or NaN patterns differ)"""
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return float("inf")
    g, r = _d(got), _d(ref)
    gn, rn = torch.isnan(g), torch.isnan(r)
    if not torch.equal(gn, rn):
        return float("inf")
    g, r = torch.nan_to_num(g), torch.nan_to_num(r)
    if torch.equal(g, r):
        return 0.0
    return max(float((g - r).abs().max() / r.abs().max().clamp_min(1e-300)), 1e-300)


def worst_rel(got, ref, atol=0.0):
    """the largest |got - ref| in excess of atol, relative to |ref| element by element (tests/test_loop_trips_gpu.py::_worst)"""
    got, ref = _d(got), _d(ref)
    err = ((got - ref).abs() - atol).clamp_min(0.0)
    rel = torch.where(err == 0, torch.zeros_like(err), err / ref.abs().clamp_min(1e-300))
    return float(rel.max()) if rel.numel() else 0.0


def grad_atol(ref):
    return 4 * EPS32 * float(_d(ref).abs().max())


def check(run, ref64):
    """Every node of the rollout from the stored values upstream of it -> [(node, what, value, bar or None)]: ``value`` is a float or
    a tuple (per element, 2-norm), ``bar`` None means the table's (bars_of).  ``ref64``: a float64 HalfUNetRef of the case's shape (it
    is loaded with the model's state BEFORE the rollout, run.state0)."""
    case, ops = run.case, run.ops
    T, K, T_in, F = case.T, case.K, case.T_in, case.F
    sdt, rdt = run.state_dtype, run.row_dtype
    forecast, train = case.mode == "forecast", case.mode != "eval"
    inference = forecast
    forced = case.strategy == "scaled_ar" and not forecast
    fig = []
    add = lambda node, what, value, bar=None: fig.append((node, what, value, bar))   # noqa: E731
    ref64 = copy.deepcopy(ref64)
    ref64.load_state_dict(run.state0)
    st0 = copy.deepcopy(ref64.state_dict())
    params, names = plan_params(st0), plan_names(st0)
    rounds = rdt == torch.bfloat16      # (the reference chain's own records are float64 in either flavour: nothing rounds)
    wq = lambda t: t.float().bfloat16().double() if rounds else t   # noqa: E731  (an operand as the matrix cores read it)
    spec = HN.Spec(bf16=rounds, training=train)
    stored_as = (lambda t: t.float().bfloat16().double()) if rounds else (lambda t: t)   # a gradient map as its producer stored it
    as_device = sdt == torch.float32
    running = [[m.clone(), v.clone()] for m, v in plan_running(st0)]
    sched = schedule(case)
    assert len(run.calls) == len(sched), f"{len(run.calls)} calls recorded, the schedule has {len(sched)}"
    states = [ops.inputs[:, t] for t in range(T_in)]      # stored states: the batch's inputs, then every recorded new state
    fws = []
    for (cc, i, k, free), rec in zip(sched, run.calls):
        tag = f"call {cc} (i={i}, k={k}{', free' if free else ''})"
        assert (rec["i"], rec["free"]) == (i, free), f"{tag}: recorded as i={rec['i']}, free={rec['free']}"
        # 1. the network input, from the stored states
        x_ref = ref_input(torch.stack(states[-T_in:], 1).to(sdt), ops.statics.to(sdt), ops.forcing[:, i].to(sdt), T_in, case.nan, run.cpad, rdt)
        add("x", f"{tag}: x", unequal(rec["x"], x_ref))
        if rec.get("x_next") is not None:
            nxt = run.calls[cc + 1]["x"]
            add("xnext", f"{tag}: emitted next input is what call {cc + 1} read", unequal(rec["x_next"], nxt))
        # the previous state the step read is the stored last state; the slot it wrote
        add("prev", f"{tag}: prev", unequal(rec["prev"], states[-1].to(sdt)))
        want_slot = ("pred", i) if k == K - 1 else ("inter", k % 2)
        add("slot", f"{tag}: new state written to {rec['slot']}, the schedule says {want_slot}", 0.0 if rec["slot"] == want_slot else float("inf"))
        # 4. the model call on the stored input
        y64, _, _ = ref_model_vjp(ref64, rec["x"], None, train, keep_stats=True)
        tgt = None if forecast else ops.outputs[:, i]
        # the call read this x: its first convolution on the stored input; its last from the stored decoder output
        fw = stored_forward(rec, case.cin, spec, as_device)
        fws.append(fw)
        y0 = HN.conv(fw.inp[0], wq(params[0]))
        add("Y0", f"{tag}: Y[0] = conv(x)", (relmax(fw.Y[0], y0), rel2(fw.Y[0], y0)) if case.bf16 else rel2(fw.Y[0], y0))
        # every later block read the input formed from the stored maps upstream of it, and this model's weights
        for j in range(1, HN.NCONV):
            yj = HN.conv(fw.inp[j], wq(params[3 * j]))
            add("Ymid", f"{tag}: Y[{j}] = conv of its input from the stored maps",
                (relmax(fw.Y[j], yj), rel2(fw.Y[j], yj)) if case.bf16 else rel2(fw.Y[j], yj))
        # the normalisation arrays: the statistics of the stored Y[j] (training, forecast), the running statistics (eval)
        stats = []
        for j in range(HN.NCONV):
            if train:
                stats.append(HN.norm_stats(fw.Y[j], spec))
                m64, v64 = stats[j][0], stats[j][1]
            else:
                m64, v64 = (HN._per_sample(s, B) for s in plan_running(st0)[j])
            arrays = HN.norm_arrays(m64, v64, params[3 * j + 1], params[3 * j + 2], spec.eps)
            for nm, got, want in zip(("scale", "shift", "mean", "rstd"), fw.norm[j], arrays):
                add("norm", f"{tag}: norm[{j}].{nm} from {'the stored Y' if train else 'the running statistics'}", rel2(got, want))
        ytail = HN.conv(spec.q(fw.A[11]), wq(params[36])).reshape(B, N, F)
        sel = (ops.interior > 0) if forced else torch.ones(N, dtype=torch.bool)
        inc_got = (_d(rec["new"]) - torch.nan_to_num(_d(rec["prev"])))[:, sel]
        inc_of = lambda y: (y.double() * (ops.std.double() if ops.std is not None else 1.0)   # noqa: E731
                            + (ops.mean.double() if ops.mean is not None else 0.0))[:, sel]
        if train:
            for j in range(HN.NCONV):
                running[j] = list(HN.running_update(running[j][0], running[j][1], stats[j][0], stats[j][2], spec.momentum))
        if rec["y"] is not None:
            got = rec["y"][..., :F]
            add("ytail", f"{tag}: y = conv1x1 of the stored decoder output", (relmax(got, ytail), rel2(got, ytail)) if case.bf16 else rel2(got, ytail))
            add("y_x", f"{tag}: y against the model re-run from x", (relmax(got, y64), rel2(got, y64)) if case.bf16 else relmax(got, y64))
            # 2. the new state from stored prev and stored y, the fp32 chain
            new_ref = ref_update(rec["prev"], rec["y"], ops.std, ops.mean, tgt, ops.border, ops.interior, case.strategy, free, inference,
                                 case.nan, sdt)
            add("state", f"{tag}: new state", unequal(rec["new"], new_ref))
        else:
            # fused tail: y is never written; the composite new - prev from the stored decoder output
            where = " on the interior" if forced else ""
            add("inc", f"{tag}: new state - prev{where}", (relmax(inc_got, inc_of(ytail)), rel2(inc_got, inc_of(ytail))))
            add("y_x", f"{tag}: new state - prev{where} against the model re-run from x", (relmax(inc_got, inc_of(y64)), rel2(inc_got, inc_of(y64))))
        # 3. the border
        if forced and case.border:
            bsel = ops.border > 0
            want = torch.nan_to_num(tgt) if case.nan else tgt
            add("border", f"{tag}: border points are the target's", unequal(rec["new"][:, bsel], want[:, bsel].to(sdt)))
        # 5. the loss of a loss step at the stored state
        if not forecast and not free:
            l_ref = ref_loss(rec["new"], tgt, ops.weights, ops.interior, ops.num_interior, ops.count, ops.kind, case.nan)
            add("loss", f"{tag}: loss[:, {i}]", worst_rel(run.loss[:, i], l_ref))
        states.append(rec["new"])
    # 6. the prediction
    for i in range(T):
        own = run.calls[i * K + K - 1]["new"]
        add("pred", f"pred[:, {i}] is the new state of call {i * K + K - 1}", unequal(run.pred[:, i], own))
        for rec in run.calls:
            if rec["c"] != i * K + K - 1 and torch.equal(torch.nan_to_num(rec["new"]), torch.nan_to_num(run.pred[:, i])):
                add("pred", f"pred[:, {i}] also equals the new state of call {rec['c']}", float("inf"))
    if not forecast:
        add("fused_loss", "fused_loss = loss * weight", unequal(run.fused_loss, run.loss * LOSS_WEIGHT))
        add("count", f"mask count {int(run.count)} against {ops.count}", 0.0 if int(run.count) == ops.count else float("inf"))
    # 7. the running statistics after T * K calls: torch's rule on the statistics of every call's stored Y[i], and (fp32) from x alone
    after = dict(ref64.named_buffers())
    stored = {}
    for j, (nm, nv) in enumerate(zip([n for n in st0 if n.endswith("running_mean")], [n for n in st0 if n.endswith("running_var")])):
        stored[nm], stored[nv] = running[j]
    for name, buf in run.buffers.items():
        if not buf.dtype.is_floating_point:
            moved = int(buf) - int(run.state0[name])
            add("nbt", f"{name} advanced by {moved}", 0.0 if moved == (T * K if train else 0) else float("inf"))
        elif train:
            add("running", name, worst_rel(buf, stored[name], 1e-5))
            add("running_x", name + " against the model re-run from x", worst_rel(buf, after[name], 1e-5))
        else:
            add("running_untouched", name, unequal(buf, run.state0[name].to(buf.dtype)))
    if case.mode != "train":
        return fig
    # ---- backward
    total64 = {}
    gp = ops.g_pred
    assert sorted(run.bwd) == list(range(T * K)), f"backward records of calls {sorted(run.bwd)}"
    dxw = NF * math.ceil(run.dxc / NF)
    for cc, i, k, free in reversed(sched):
        rec, b = run.calls[cc], run.bwd[cc]
        tag = f"call {cc} (i={i}, k={k}{', free' if free else ''})"
        last = cc == T * K - 1
        assert b["free"] == free and b["i"] == i, f"{tag}: backward recorded as i={b['i']}, free={b['free']}"
        # 8. what arrives at the new state
        if T_in == 1:
            want = None if last else run.bwd[cc + 1]["dprev"]
            if gp is not None and k == K - 1:
                want = gp[:, i].to(sdt) if want is None else want + gp[:, i].to(sdt)
            if want is None or b["g_next"] is None:
                add("gnext", f"{tag}: g_next {'present' if b['g_next'] is not None else 'absent'}",
                    0.0 if (want is None) == (b["g_next"] is None) else float("inf"))
            else:
                add("gnext", f"{tag}: g_next = dprev of call {cc + 1}{' + g_pred' if gp is not None and k == K - 1 else ''}", unequal(b["g_next"], want))
            want2 = None if last else run.bwd[cc + 1]["dx"]
            if want2 is None or b["g_next2"] is None:
                add("gnext2", f"{tag}: g_next2 {'present' if b['g_next2'] is not None else 'absent'}",
                    0.0 if (want2 is None) == (b["g_next2"] is None) else float("inf"))
            else:
                add("gnext2", f"{tag}: g_next2 = dx of call {cc + 1}", unequal(b["g_next2"], want2))
        else:
            want_parts = expected_parts(case, i, gp is not None)
            add("parts", f"{tag}: parts {b['parts']}, the window says {want_parts}", 0.0 if list(b["parts"] or []) == want_parts else float("inf"))
            tensors = []
            for kind, kk, off in want_parts:
                tensors.append((gp[:, i].to(sdt), 0) if kind == "gpred" else (run.bwd[kk]["dprev"], 0) if kind == "dprev" else (run.bwd[kk]["dx"], off))
            if tensors and b["g_next"] is not None:
                add("gsum", f"{tag}: gsum", unequal(b["g_next"], ref_state_grad_sum(tensors, F, sdt)))
            else:
                add("gsum", f"{tag}: gsum {'present' if b['g_next'] is not None else 'absent'}",
                    0.0 if bool(tensors) == (b["g_next"] is not None) else float("inf"))
            add("gnext2", f"{tag}: no rows of an input gradient", 0.0 if b["g_next2"] is None else float("inf"))
        lg = None if (run.lgrads is None or free) else run.lgrads[i]
        if lg is not None:
            # the saved loss gradient row i is d loss_elem / d pred at the stored new state of THIS step: one rounding of the rows' type
            add("lgrad", f"{tag}: saved loss gradient lgrads[{i}]", worst_rel(lg, 2.0 * (_d(rec["new"]) - _d(ops.outputs[:, i]))))
        dy_ref, dp_ref = ref_step_adjoint(rec["prev"], rec["y"], rec["new"], ops.outputs[:, i], ops, case, free, ops.gl[:, i],
                                          b["g_next"], b["g_next2"], lgrad=lg, ycs=b["dy"].shape[-1])
        add("dy", f"{tag}: dy", worst_rel(b["dy"], dy_ref, grad_atol(dy_ref)))
        add("dyzero", f"{tag}: channels >= F of dy", float(b["dy"][..., F:].double().abs().max()) if b["dy"].shape[-1] > F else 0.0)
        if cc > 0:
            ok = ~torch.isnan(rec["prev"])
            add("dprev", f"{tag}: dprev", worst_rel(b["dprev"][ok], dp_ref[ok], grad_atol(dp_ref)))
        else:
            add("sentinel", f"{tag}: dprev untouched", 0.0 if b["dprev_untouched"] and b["dprev"] is None else float("inf"))
            add("sentinel", f"{tag}: dx untouched", 0.0 if b["dx0_untouched"] and b["dx"] is None else float("inf"))
        # 9. the model call's data gradient from stored x, dy and the call's stored forward maps (every decision the device's)
        dx_full, grads = stored_backward(fws[cc], params, spec, b["dy"][..., :F].reshape(B, H, W, F), stored_as)
        for n, g in zip(names, grads):
            total64[n] = g if n not in total64 else total64[n] + g
        if cc > 0:
            got = b["dx"]
            assert got.shape[-1] == dxw, f"{tag}: dx rows of {got.shape[-1]} channels, the plan says {dxw}"
            dx64 = dx_full.reshape(B, N, case.cin)[..., :run.dxc]
            add("dx", f"{tag}: dx", (relmax(got[..., :run.dxc], dx64), rel2(got[..., :run.dxc], dx64)) if case.bf16 else relmax(got[..., :run.dxc], dx64))
            # (channels dx_channels .. cin - 1 of the last block are not the sweep's to read: the plan leaves the other inputs' gradient there)
            add("dxzero", f"{tag}: channels >= {case.cin} of dx (padded input channels)",
                float(got[..., case.cin:].double().abs().max()) if dxw > case.cin else 0.0)
    # 10. every parameter gradient is the sum of its calls'
    assert set(run.pgrads) == set(total64), "every parameter has a gradient"
    for n, g in run.pgrads.items():
        add("pgrad", f"grad of {n}", rel2(g, total64[n].reshape(g.shape)) if case.bf16 else relmax(g, total64[n].reshape(g.shape)))
    return fig


def judge(case, fig):
    """(failures, worst): every figure against its bar; worst = {node: (value, bar, what)} by the figure's last component"""
    bars = bars_of(case)
    failures, worst = [], {}
    for node, what, value, bar in fig:
        bar = bars[node] if bar is None else bar
        vals = value if isinstance(value, tuple) else (value,)
        lims = bar if isinstance(bar, tuple) else (bar,) * len(vals)
        for j, (v, lim) in enumerate(zip(vals, lims)):
            key = node if len(vals) == 1 else f"{node} ({('per element', '2-norm')[j]})"
            if v >= worst.get(key, (-1.0,))[0]:
                worst[key] = (v, lim, what)
            if not v <= lim:
                failures.append(f"{what}: {node} {v:.3e} > {lim:.1e}")
    return failures, worst


def node_value(fig, node):
    """the worst value a node shows in a set of figures (the last component of a two-figure node)"""
    vals = [(v[-1] if isinstance(v, tuple) else v) for n, _, v, _ in fig if n == node]
    return max(vals) if vals else 0.0


# ------------------------------------------------------------------------------------------------ the recorder
class Recorder:
    """Context manager: replaces the module-level functions of py4cast_amd/halfunet_rollout.py that name the native calls by wrappers
    which call the original and then clone, on the same stream, what the call wrote; ``_lib.call`` is wrapped for the entry points'
    names (and the part list of p4c_sum_state_grads).  Buffers a call must not touch are filled with a sentinel first.  Everything is
    restored on exit."""

    NAMES = ("_build_x", "_model_forward", "_free_step", "_loss_step", "_step_backward", "_model_backward", "_finish_sweep", "_sweep",
             "_sweep_window")

    def __init__(self):
        self.calls, self.bwd, self.entries = [], [], []
        self.r = self.w = self.g_pred = self.gl = self.loss = None
        self.ops, self.inter, self.parts, self.built = {}, [], None, None
        self.finished = False

    def __enter__(self):
        from py4cast_amd import _lib as L
        from py4cast_amd import halfunet_rollout as HR

        self.HR, self.L = HR, L
        self.orig = {n: getattr(HR, n) for n in self.NAMES}
        self.orig_call = L.call
        try:
            L.call = self._call
            for n in self.NAMES:
                setattr(HR, n, getattr(self, "_w" + n))
        except BaseException:
            self.undo()
            raise
        return self

    def __exit__(self, *exc):
        self.undo()
        return False

    def undo(self):
        try:
            for n, f in self.orig.items():
                setattr(self.HR, n, f)
        finally:
            self.L.call = self.orig_call

    # ---- the library's entry points
    def _call(self, name, *args, **kwargs):
        self.entries.append(name)
        if name == "p4c_sum_state_grads":
            n = args[2]
            self.parts = [(int(args[3][j] or 0), int(args[4][j]), int(args[5][j]), int(args[6][j]), int(args[7][j])) for j in range(n)]
        return self.orig_call(name, *args, **kwargs)

    def _take(self):
        e, self.entries = self.entries, []
        return e

    def _first(self, r):
        if self.r is not r:
            self.r = r
            self.ops = {n: getattr(r, n) for n in ("inputs", "forcing", "statics", "std", "mean", "outputs", "border", "interior", "weights",
                                                   "count", "loss")}
            self.inter = list(r.inter)

    # ---- forward
    def _w_build_x(self, r, i, prev, sbs_prev, x):
        self._first(r)
        self.orig["_build_x"](r, i, prev, sbs_prev, x)
        self.built = x.data_ptr()

    def _w_model_forward(self, r, x, saved):
        self._first(r)
        rec = dict(c=len(self.calls), x=x.detach().clone(), x_ptr=x.data_ptr(), built=self.built == x.data_ptr(), saved_ptr=saved.data_ptr())
        self.built = None
        self.orig["_model_forward"](r, x, saved)
        rec["y"] = None if r.fused_tail else r.y.detach().clone()
        rec["saved"] = saved.detach().clone()
        rec["entries"] = self._take()
        self.calls.append(rec)

    def _step(self, name, free, r, i, saved, prev, sbs_prev, new, sbs_new, x_next, forcing_next):
        rec = self.calls[-1]
        rec.update(i=i, free=free, prev=prev.detach().clone(), new_ptr=new.data_ptr(), step=name)
        self.orig[name](r, i, saved, prev, sbs_prev, new, sbs_new, x_next, forcing_next)
        rec["new"] = new.detach().clone()
        rec["x_next"] = None if x_next is None else x_next.detach().clone()
        rec["entries"] += self._take()

    def _w_free_step(self, *a):
        self._step("_free_step", True, *a)

    def _w_loss_step(self, *a):
        self._step("_loss_step", False, *a)

    # ---- backward
    def _w_sweep(self, r, w, g_pred):
        self._sweep("_sweep", r, w, g_pred)

    def _w_sweep_window(self, r, w, g_pred):
        self._sweep("_sweep_window", r, w, g_pred)

    def _sweep(self, name, r, w, g_pred):
        self.w, self.sweep = w, name
        self.g_pred = None if g_pred is None else g_pred.detach().clone()
        self.g_pred_contig = g_pred is not None and g_pred.dtype == torch.float32 and g_pred.is_contiguous()
        self.g_pred_ptr = None if g_pred is None else g_pred.data_ptr()
        self.gl = None if w.gl is None else w.gl.detach().clone()
        self._take()
        self.orig[name](r, w, g_pred)

    def _w_step_backward(self, r, w, i, free, g_next, g_next2, dprev):
        b = dict(i=i, free=free, g_next=None if g_next is None else g_next.detach().clone(),
                 g_next2=None if g_next2 is None else g_next2.detach().clone(), raw_parts=self.parts, dprev_untouched=True, dx0_untouched=True)
        self.parts = None
        pre = self._take()
        snap = None
        if dprev is None:
            if g_next is None or g_next.data_ptr() != w.dprev.data_ptr():
                w.dprev.fill_(SENT)
            snap = w.dprev.detach().clone()
        self.orig["_step_backward"](r, w, i, free, g_next, g_next2, dprev)
        b["dy"] = w.dy.detach().clone()
        b["dprev"] = None if dprev is None else dprev.detach().clone()
        if snap is not None:
            b["dprev_untouched"] = torch.equal(snap, w.dprev)
        b["entries"] = pre + self._take()
        self.bwd.append(b)

    def _w_model_backward(self, r, w, c, dx):
        b = self.bwd[-1]
        b["c"] = c
        if dx is not None:
            dx.fill_(SENT)
        self.orig["_model_backward"](r, w, c, dx)
        b["dx"], b["dx_ptr"] = None, None
        if dx is not None and c > 0:
            b["dx"], b["dx_ptr"] = dx.detach().clone(), dx.data_ptr()
        elif dx is not None:
            b["dx0_untouched"] = untouched(dx)
        b["entries"] += self._take()

    def _w_finish_sweep(self, r, w):
        out = self.orig["_finish_sweep"](r, w)
        self.finished = True
        return out

    # ---- the records in the checker's format
    def slot_of(self, ptr):
        r = self.r
        for i in range(r.T):
            if r.pred[:, i].data_ptr() == ptr:
                return ("pred", i)
        for j, t in enumerate(self.inter):
            if t.data_ptr() == ptr:
                return ("inter", j)
        return ("unknown", ptr)

    def label_parts(self, b, later):
        """the raw (pointer, batch stride, channel stride, offset, type) parts of a p4c_sum_state_grads call by the buffer each points at:
        dprev, the dx buffer (by the call that wrote it LAST before this point of the sweep), or the prediction's gradient"""
        if b["raw_parts"] is None:
            return []
        r, w = self.r, self.w
        dxw = NF * ((r.desc.dx_channels + NF - 1) // NF)
        out = []
        for ptr, bs, cs, off, dt in b["raw_parts"]:
            writers = [x for x in later if x.get("dx_ptr") == ptr]
            if ptr == w.dprev.data_ptr():
                ok = (bs, cs, off, dt) == (r.N * r.F, r.F, 0, self.L.F32)
                out.append(("dprev" if ok else "dprev-misdescribed", b["i"] + 1, off))
            elif writers:
                ok = (bs, cs, dt) == (r.N * dxw, dxw, r.acode)
                out.append(("dx" if ok else "dx-misdescribed", writers[-1]["c"], off))
            else:
                ok = (cs, off, dt) == (r.F, 0, self.L.F32) and self.g_pred is not None
                if ok and self.g_pred_contig:
                    ok = ptr == self.g_pred_ptr + b["i"] * r.N * r.F * 4 and bs == r.T * r.N * r.F
                out.append(("gpred" if ok else "unknown", b["i"], off))
        return out

    def to_run(self, case, lm, state0, pred, fused_loss):
        """the records on the CPU, flat"""
        r = self.r
        cpu = lambda t: None if t is None else t.detach().cpu()   # noqa: E731
        rows = lambda t: None if t is None else cpu(t).reshape(t.shape[0], -1, t.shape[-1])   # noqa: E731
        o = self.ops
        statics = cpu(o["statics"]).reshape(-1, r.N, r.Fs)
        ops = SimpleNamespace(
            inputs=cpu(o["inputs"]).reshape(B, case.T_in, N, case.F), forcing=cpu(o["forcing"]).reshape(B, case.T, N, case.Ff),
            outputs=None if o["outputs"] is None else cpu(o["outputs"]).reshape(B, case.T, N, case.F),
            statics=statics.expand(B, N, case.Fs), std=cpu(o["std"]), mean=cpu(o["mean"]),
            border=None if o["border"] is None else cpu(o["border"]).reshape(N).float(),
            interior=None if o["interior"] is None else cpu(o["interior"]).reshape(N).float(),
            weights=cpu(o["weights"]), num_interior=float(r.num_interior), kind="mse" if r.kind == 0 else "l1",
            count=0 if r.count is None else int(r.count), gl=cpu(self.gl), g_pred=None if self.g_pred is None else rows4(cpu(self.g_pred)))
        from py4cast_amd import ops_model as om

        lay = om.halfunet_layout(r.desc)
        assert lay["saved_bytes"] == r.saved_bytes
        shape = [(B, H >> k, W >> k, NF) for k in range(HN.NLEV)]
        calls = []
        for rec in self.calls:
            sv = rec["saved"]
            stored_y = [cpu(HN._view(sv, lay["Y"][j], r.adt, shape[HN.LEVEL[j]])).clone() for j in range(HN.NCONV)]
            stored_norm = [tuple(cpu(HN._view(sv, lay["norm"][j] + q * B * NF * 4, torch.float32, (B, NF))).clone() for q in range(4))
                           for j in range(HN.NCONV)]
            calls.append(dict(c=rec["c"], i=rec["i"], k=rec["c"] % case.K, free=rec["free"], x=rows(rec["x"]), x_next=rows(rec["x_next"]),
                              Y=stored_y, norm=stored_norm,
                              y=rows(rec["y"]), prev=rows(rec["prev"]), new=rows(rec["new"]), slot=self.slot_of(rec["new_ptr"]),
                              entries=rec["entries"], built=rec["built"], x_ptr=rec["x_ptr"], saved_ptr=rec["saved_ptr"], step=rec["step"]))
        bwd = {}
        for j, b in enumerate(self.bwd):
            bwd[b["c"]] = dict(c=b["c"], i=b["i"], free=b["free"], g_next=rows(b["g_next"]), g_next2=rows(b["g_next2"]), dy=rows(b["dy"]),
                               dprev=rows(b["dprev"]), dx=rows(b["dx"]), dx_ptr=b["dx_ptr"], dprev_untouched=b["dprev_untouched"],
                               dx0_untouched=b["dx0_untouched"], entries=b["entries"],
                               parts=self.label_parts(b, self.bwd[:j]) if case.T_in > 1 else None)
        model = lm.model
        return SimpleNamespace(
            case=case, ops=ops, calls=calls, bwd=bwd, pred=rows4(cpu(pred)), loss=cpu(self.ops["loss"]), fused_loss=cpu(fused_loss),
            lgrads=None if r.lgrads is None else cpu(r.lgrads).reshape(case.T, B, N, case.F), cpad=r.cpad, dxc=int(r.desc.dx_channels),
            state_dtype=torch.float32, row_dtype=r.adt, state0=state0, buffers={k: cpu(v).clone() for k, v in model.named_buffers()},
            pgrads={n: cpu(p.grad).clone() for n, p in model.named_parameters()} if case.mode == "train" else None,
            count=0 if r.count is None else int(r.count), fused_tail=bool(r.fused_tail), training=bool(r.training),
            save_lg=bool(r.save_lg), fuse_next=bool(r.fuse_next), feed=bool(r.feed), sweep=getattr(self, "sweep", None), finished=self.finished)


def rows4(t):
    """(B, T, H, W, F) or (B, T, N, F) -> (B, T, N, F)"""
    return None if t is None else t.reshape(t.shape[0], t.shape[1], -1, t.shape[-1])


# ------------------------------------------------------------------------------------------------ one case on the device
BF16 = {"compute_dtype": "bf16", "activation_dtype": "bf16"}


def make_lm(case, c, device):
    from helpers import make_dataset_info
    from py4cast_amd.lightning import AutoRegressiveLightning

    info = make_dataset_info(c, case.Ff)
    torch.manual_seed(0)
    return AutoRegressiveLightning(
        BF16 if case.bf16 else {}, info, None, num_input_steps=case.T_in, num_pred_steps_train=case.T, batch_size=B, model_name="HalfUNet",
        losses=[{"class": "WeightedLoss", "weight": LOSS_WEIGHT, "params": {"loss": "MSELoss", "reduction": "none"}}],
        training_strategy=case.strategy, mask_on_nan=case.nan, num_inter_steps=case.K,
    ).to(device)


def forecast_batch(case, c, device):
    from helpers import GRID_DIMS, feature_names
    from py4cast_amd.base import ItemBatch
    from py4cast_amd.namedtensor import NamedTensor

    return ItemBatch(NamedTensor(c["inputs"].clone().to(device), GRID_DIMS, feature_names(case.F)),
                     NamedTensor(c["forcing"].clone().to(device), GRID_DIMS, [f"g{i}" for i in range(case.Ff)]), None)


def device_run(name, device, before=None):
    """One rollout of the case under the recorder: training_step + backward() (train), common_step under no_grad on the .eval() model
    (eval), common_step(..., "inference") on the .train() model (forecast) -> (run, lm, recorder, the case's tensors).
    ``before(lm)`` runs right ahead of the recorded rollout (e.g. to pre-fill the parameter gradients)."""
    from helpers import make_batch

    case = CASES[name]
    c = case_inputs(case)
    lm = make_lm(case, c, device)
    lm.use_native_rollout = True
    lm.train()
    with torch.no_grad():   # non-trivial affine parameters
        for nb in lm.model._norms:
            nb.weight.uniform_(0.5, 1.5)
            nb.bias.uniform_(-0.3, 0.3)
    if case.mode != "train":
        lm.training_step(make_batch(c, device), 0)   # records the names, moves the running statistics off their initial values
        lm.zero_grad(set_to_none=True)
    if case.mode == "eval":
        lm.eval()
    if before is not None:
        before(lm)
    torch.cuda.synchronize()
    state0 = {k: v.detach().cpu().clone() for k, v in lm.model.state_dict().items()}
    with Recorder() as rec:
        if case.mode == "train":
            if case.gpred:
                pred, _ = lm.common_step(make_batch(c, device), 0, "train")
                fused = pred.fused_loss
                assert fused is not None, f"{name}: the native rollout was not taken"
                loss = torch.mean(fused) + GPRED * (rows4(pred.tensor) * gpred_weights(case).to(device)).sum()
                ptensor = pred.tensor
            else:
                got = {}
                real = lm.common_step

                def spy(*a, **kw):
                    out = real(*a, **kw)
                    got["pred"] = out[0]
                    return out

                lm.common_step = spy
                try:
                    loss = lm.training_step(make_batch(c, device), 0)
                finally:
                    del lm.common_step
                fused, ptensor = got["pred"].fused_loss, got["pred"].tensor
                assert fused is not None, f"{name}: the native rollout was not taken"
            loss.backward()
        elif case.mode == "eval":
            with torch.no_grad():
                pred, _ = lm.common_step(make_batch(c, device), 0, "val")
            fused, ptensor = pred.fused_loss, pred.tensor
            assert fused is not None, f"{name}: the native rollout was not taken"
        else:
            with torch.no_grad():
                pred, _ = lm.common_step(forecast_batch(case, c, device), 1, "inference")
            fused, ptensor = None, pred.tensor
        torch.cuda.synchronize()
        assert rec.calls, f"{name}: the native rollout was not taken (no native call recorded)"
        run = rec.to_run(case, lm, state0, ptensor.detach(), None if fused is None else fused.detach())
    return run, lm, rec, c
