"""
Native rollout of the HalfUNet (``HalfUNetMI355X.native_rollout``): the schedule of T * K model calls of
AutoRegressiveLightning._common_step (lightning.py:565-662) enqueued from Python -- per call p4c_build_x (or the previous step's
fused next input) -> HalfUNet plan -> AR step (state update + border forcing, with or without the weighted loss) -- as ONE autograd
node (``_NativeRolloutFn``: training / validation, with the matching reverse sweep) or as a forward-only forecast
(``native_forecast``: phase "inference").

Auto-padded grids (``autopad_enabled``, a grid that is not a multiple of 16; one input state, one model call per target step): the
NETWORK side -- x, the plan's maps, y, dy, dx -- lives on the padded grid (B, Hp, Wp, ..), the STATE side -- the batch's tensors, the
masks, the prediction, dprev, g_pred, the loss workspace -- stays at (B, H, W, ..) and is never copied or padded.  ``_Rollout.window``
= (Hp, Wp, top, left) says so, and the four calls that connect the two sides take the ``_win`` entry points of csrc/rollout_win.hip,
which address through the window: state pixel (h, w) is network row (top + h) * Wp + left + w.  No fused next input, no fused 1x1
tail, no saved loss gradients there: p4c_build_x_win runs per model call and the plan writes y.

Every decision exists once: ``_Rollout`` is what a rollout passes around, ``_schedule`` maps a call index to its states, and each
kind of native call (``_build_x``, ``_model_forward``, ``_free_step``, ``_loss_step``, ``_step_backward``, ``_model_backward``) is the
only place that names its entry points and lays out their arguments.
"""

import ctypes
from types import SimpleNamespace

import torch

from . import _lib as L
from ._lib_model import HalfUNetDesc
from .halfunet import NF


def _step_paths(model, T_in, N, F, Fs, mask_on_nan):
    """(feed, v4_next, flat_next): whether the AR step's kernel also writes the next network input ("feed next step": one input
    state, otherwise p4c_build_x builds the window), and which of the step kernels' two fast paths the shape takes -- the conditions
    of csrc/losses.hip, stated once for the training rollout and the forecast."""
    cpad = model.cin_pad
    feed = T_in == 1
    lanes = 1
    while lanes < F // 4:
        lanes *= 2  # lanes per grid point of the 16-byte update kernel; each also owns one tail quad of x_next
    v4_next = ((not mask_on_nan) and F % 4 == 0 and F <= 64
               and (not feed or (Fs % 4 == 0 and cpad % 4 == 0 and cpad // 4 - F // 4 <= lanes)))
    # any other feature count (the shipped Titan configuration has 21 features): the flat kernels of csrc/losses.hip -- (N, F)
    # arrays streamed flat, the network's row tensors through LDS tiles -- take the same fused step
    esz = 2 if model.act_dtype == torch.bfloat16 else 4
    flat_next = ((not mask_on_nan) and F <= 64 and (N * F) % 4 == 0 and (cpad * esz) % 16 == 0 and cpad <= 256
                 and L.diag_switch("P4C_NO_FLAT_STEP") != "1")
    return feed, v4_next, flat_next


def padded_grid_is_native(padding, autopad_enabled, T_in, K, channels, in_channels):
    """Whether a rollout on a grid the network has to pad (``padding`` = HalfUNetMI355X.padding_for(H, W), not all zero) takes the
    native route: only with ``autopad_enabled`` (otherwise ``forward`` raises, through the generic route), ONE input state (T_in >= 2
    needs a windowed p4c_sum_state_grads), ONE model call per target step, and the batch's channel count
    (T_in * F + statics + forcing + NaN-mask channel) equal to the network's.  A grid that fits is not this function's question."""
    return bool(any(padding) and autopad_enabled and T_in == 1 and K == 1 and channels == in_channels)


def _fused_tail(model, v4_next, flat_next, F, mask_on_nan):
    """bf16 flavour: the network's 1x1 output convolution runs INSIDE the AR step's kernel (p4c_out_conv_update_loss_fwd /
    p4c_out_conv_update_fwd: y is never written and read back, one launch less per AR step; same new state bit for bit;
    P4C_FUSED_TAIL=0: the two-kernel route).  (Feature counts off the 16-byte grid: the flat kernel takes the convolution as its
    front end.)"""
    return (model.act_dtype == torch.bfloat16 and (v4_next or (flat_next and F % 4 != 0)) and not mask_on_nan
            and model.out_channels >= F and L.diag_switch("P4C_FUSED_TAIL") != "0")


class _Rollout:
    """What one rollout passes around.  ``_rollout_context`` builds it once with
      model, desc (the plan the backward uses too), desc_fwd (the forward's: skip_out_conv with the fused tail), flat, scratch,
      saved_bytes, B, T, T_in, K, H, W, N, F, Fs, Ff, cpad, inputs, forcing, statics + sbs_statics (batch stride 0 when every
      sample shares them), std, mean, mask_on_nan, adt / acode (activation dtype and its code), stream, training,
      window (None, or (Hp, Wp, top, left) of an auto-padded grid) with Hn, Wn (the network's grid: Hp, Wp or H, W) and win_args (what
      the _win entry points take ahead of the stream),
      feed (one input state), fuse_next (the step's kernel writes the next network input), step_capable (one of the step kernels'
      two fast paths applies), fused_tail (the 1x1 output convolution runs inside the step's kernel);
    the callers add what is listed below.  The reverse sweep reads it again; ``release_forward`` drops what only the forward needs."""

    # state slots (``_state_slots``): pred[:, i] = new state of AR step i, batch stride sbs_state; states = the (T_in + T)-slot buffer
    # pred is a view of, where there is one; inter = scratch ring for the intermediary states of K >= 2; y = the plan's output rows
    states = pred = y = None
    sbs_state = 0
    # the loss-carrying steps (training / validation node only: a forecast has loss = None and forces no border)
    outputs = border = interior = weights = count = loss = ws = lgrads = None
    sbs_out = kind = 0
    num_interior = 0.0
    mask_mode = L.MASK_NONE
    force_border = save_lg = False

    def __init__(self, **fields):
        self.__dict__.update(fields)
        self.inter, self.xs, self.saveds = [], [], []   # xs / saveds: activations kept per call for the reverse sweep

    def release_forward(self):
        for name in ("inputs", "forcing", "statics", "mean", "border", "y", "ws", "loss", "inter", "flat", "scratch", "desc_fwd"):
            setattr(self, name, None)


def _rollout_context(model, inputs, forcing, statics, std, mean, T, K, mask_on_nan, training, node):
    """The part of the set-up the training node and the forecast share.  ``node``: the plan also serves a reverse sweep (its input
    gradient is what the sweep reads)."""
    dev = inputs.device
    B, T_in, H, W, F = inputs.shape
    N = H * W
    Fs, Ff = statics.shape[-1], forcing.shape[-1]
    st = statics.float()
    sbs = 0 if st.stride(0) == 0 else N * Fs
    st = st[0].contiguous() if sbs == 0 else st.contiguous()
    top, bottom, left, right = model.padding_for(H, W)
    window = (H + top + bottom, W + left + right, top, left) if (top or bottom or left or right) else None
    Hn, Wn = window[:2] if window else (H, W)
    desc = model._desc(B, Hn, Wn)
    if node and T_in > 1:
        desc.dx_channels = T_in * F   # the window of past states: the gradient the sweep reads
    elif node and desc.dx_channels > NF:
        desc.dx_channels = F   # one input state (F <= out_channels <= 64): its gradient is all the sweep reads
    flat = model._flat_params()
    saved_bytes, scratch = model._workspaces(desc, dev)
    # "feed next step" fused: the update kernel of step i also writes step i+1's network input (new state | statics |
    # next forcing | padding), so only step 0 runs p4c_build_x.  (The NaN-mask input channel needs p4c_build_x.)
    # (T_in >= 2: the next input is a window of several states, built by p4c_build_x; the update kernels run without x_next)
    feed, v4_next, flat_next = _step_paths(model, T_in, N, F, Fs, mask_on_nan)
    fused_tail = _fused_tail(model, v4_next, flat_next, F, mask_on_nan)
    if window:
        # the step kernels behind the window emit no next input, save no loss gradient and take y from the plan
        v4_next = flat_next = fused_tail = False
    desc_fwd = desc
    if fused_tail:
        desc_fwd = HalfUNetDesc.from_buffer_copy(desc)
        desc_fwd.skip_out_conv = 1
    return _Rollout(model=model, desc=desc, desc_fwd=desc_fwd, flat=flat, scratch=scratch, saved_bytes=saved_bytes, B=B, T=T, T_in=T_in,
                    K=K, H=H, W=W, Hn=Hn, Wn=Wn, window=window, win_args=(H, W, Hn, Wn, top, left), N=N, F=F, Fs=Fs, Ff=Ff,
                    cpad=model.cin_pad, inputs=inputs, forcing=forcing, statics=st,
                    sbs_statics=sbs, std=std, mean=mean, mask_on_nan=mask_on_nan, adt=model.act_dtype,
                    acode=L.dtype_code(model.act_dtype), stream=L.stream(dev), training=training, feed=feed,
                    fuse_next=feed and (v4_next or flat_next), step_capable=v4_next or flat_next, fused_tail=fused_tail)


def _prepare_weights(r):
    # the parameters are fixed for the whole rollout: re-lay / round the weights once, not once per AR step
    L.call("p4c_halfunet_prepare_weights", ctypes.byref(r.desc), L.ptr(r.flat), L.ptr(r.scratch), r.stream)
    r.desc.weights_prepared = 1
    r.desc_fwd.weights_prepared = 1


def _state_slots(r, window):
    """Where state slot i lives.  ``window``: a (T_in + T)-slot buffer -- slots 0 .. T_in-1 the input states (copied once for
    T_in >= 2; with one input state slot 0 is never written: AR step 0 reads the batch's input state where it lies, every kernel takes
    the previous state's batch stride separately, which saves a 126 MB copy per rollout at the benchmark size), slot T_in + i the new
    state of AR step i, the input of step i the window of slots i .. i+T_in-1.  Otherwise (a forecast of one input state): the T-slot
    result alone."""
    dev = r.inputs.device
    if window:
        r.states = torch.empty(r.B, r.T_in + r.T, r.H, r.W, r.F, dtype=torch.float32, device=dev)
        if r.T_in > 1:
            r.states[:, :r.T_in].copy_(r.inputs)
        r.pred, r.sbs_state = r.states[:, r.T_in:], (r.T_in + r.T) * r.N * r.F
    else:
        r.pred, r.sbs_state = torch.empty(r.B, r.T, r.H, r.W, r.F, dtype=torch.float32, device=dev), r.T * r.N * r.F


def _schedule(r, c):
    """Call c of the T * K -> (i, k, prev, prev's batch stride, new, new's batch stride).  Call (i, k) with k < K - 1 is an
    intermediary step: its state is not part of the prediction (lightning.py:583-658) and goes to a scratch ring of two buffers;
    call (i, K - 1) writes prediction slot i."""
    i, k = divmod(c, r.K)
    state_sz = r.N * r.F
    if not r.feed:
        prev, sbs_prev = r.states[:, i + r.T_in - 1], r.sbs_state
    elif c == 0:
        prev, sbs_prev = r.inputs[:, 0], r.T_in * state_sz
    elif k == 0:
        prev, sbs_prev = r.pred[:, i - 1], r.sbs_state
    else:
        prev, sbs_prev = r.inter[(k - 1) % 2], state_sz
    new, sbs_new = (r.pred[:, i], r.sbs_state) if k == r.K - 1 else (r.inter[k % 2], state_sz)
    return i, k, prev, sbs_prev, new, sbs_new


def _new_x(r):
    return torch.empty(r.B, r.Hn, r.Wn, r.cpad, dtype=r.adt, device=r.inputs.device)


def _build_x(r, i, prev, sbs_prev, x):
    win, sbs_win = (prev, sbs_prev) if r.feed else (r.states[:, i], r.sbs_state)
    args = (L.ptr(win), sbs_win, r.N * r.F, L.ptr(r.statics), r.sbs_statics, L.ptr(r.forcing[:, i]), r.T * r.N * r.Ff,
            L.ptr(x), r.acode, r.cpad, r.B, r.T_in, r.N, r.F, r.Fs, r.Ff, r.mask_on_nan, 0)
    if r.window:
        L.call("p4c_build_x_win", *args, *r.win_args, r.stream)   # every element of x: zeros outside the window, no memset
    else:
        L.call("p4c_build_x", *args, r.stream)


def _model_forward(r, x, saved):
    L.call("p4c_halfunet_forward", ctypes.byref(r.desc_fwd), L.ptr(x), L.ptr(r.flat), L.ptr(r.model._running),
           None if r.fused_tail else L.ptr(r.y), L.ptr(saved), L.ptr(r.scratch), int(r.training), r.stream)


def _tail(r, saved):
    """(a, scale, shift, w): what the fused tail reads of the plan -- the last block's raw output, its normalisation, the 1x1 weight"""
    ta, tsc, tsh, tw = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    L.call("p4c_halfunet_tail", ctypes.byref(r.desc_fwd), L.ptr(r.flat), L.ptr(saved), ctypes.byref(ta), ctypes.byref(tsc),
           ctypes.byref(tsh), ctypes.byref(tw))
    return ta, tsc, tsh, tw, r.model.out_channels


def _next_input(r, x_next, forcing_next):
    return (L.ptr(x_next), r.cpad, L.ptr(r.statics), r.sbs_statics, r.Fs, L.ptr(forcing_next), r.T * r.N * r.Ff, r.Ff)


def _free_step(r, i, saved, prev, sbs_prev, new, sbs_new, x_next, forcing_next):
    """One AR step without a loss term (an intermediary call of num_inter_steps >= 2, an inference call): the update, the border
    forcing where the rollout forces one, optionally the next network input -- behind the fused 1x1 output convolution where the
    fused tail applies."""
    force = r.force_border
    update = (L.ptr(r.outputs[:, i] if force else None), r.sbs_out, L.ptr(r.std), L.ptr(r.mean), L.ptr(r.border if force else None),
              L.ptr(r.interior if force else None), L.ptr(new), sbs_new)
    if r.window:
        L.call("p4c_ar_update_next_win", L.ptr(prev), sbs_prev, L.ptr(r.y), r.acode, NF, *update, int(r.mask_on_nan), r.B, r.N, r.F, 1.0,
               *r.win_args, r.stream)
    elif r.fused_tail:
        L.call("p4c_out_conv_update_fwd", *_tail(r, saved), L.ptr(prev), sbs_prev, *update, r.B, r.N, r.F, 1.0,
               *_next_input(r, x_next, forcing_next), r.stream)
    else:
        L.call("p4c_ar_update_next", L.ptr(prev), sbs_prev, L.ptr(r.y), r.acode, NF, *update, int(r.mask_on_nan), r.B, r.N, r.F, 1.0,
               *_next_input(r, x_next, forcing_next), r.stream)


def _loss_step(r, i, saved, prev, sbs_prev, new, sbs_new, x_next, forcing_next):
    """The loss-carrying AR step: update + border forcing + weighted loss of prediction slot i, optionally the next network input
    (x_next) and the saved loss gradient (save_lg)."""
    update = (L.ptr(r.outputs[:, i]), r.sbs_out, L.ptr(r.std), L.ptr(r.mean), L.ptr(r.border if r.force_border else None),
              L.ptr(r.interior), L.ptr(new), sbs_new, L.ptr(r.weights), r.num_interior, L.ptr(r.count), r.kind)
    loss = (L.ptr(r.loss[:, i]), r.T, L.ptr(r.ws), r.B, r.N, r.F, 1.0)
    nxt = _next_input(r, x_next, forcing_next)
    lgrad = (L.ptr(r.lgrads[i]) if r.save_lg else None, r.N * r.F)
    if r.fused_tail:
        L.call("p4c_out_conv_update_loss_fwd", *_tail(r, saved), L.ptr(prev), sbs_prev, *update, *loss, *nxt, *lgrad, r.stream)
        return
    step = (L.ptr(prev), sbs_prev, L.ptr(r.y), r.acode, NF, *update, r.mask_mode, *loss)
    if r.window:
        L.call("p4c_ar_update_loss_fwd_win", *step, *r.win_args, r.stream)
    elif r.save_lg:
        L.call("p4c_ar_update_loss_fwd_next_saved", *step, *nxt, *lgrad, r.stream)
    elif x_next is not None:
        L.call("p4c_ar_update_loss_fwd_next", *step, *nxt, r.stream)
    else:
        L.call("p4c_ar_update_loss_fwd", *step, r.stream)


def _run_schedule(r, xring, keep_saved):
    """The T * K model calls.  Call (i, k) is a FREE step for k < K - 1 -- forced to outputs[:, i] at the border, no loss, and its next
    input takes forcing[:, i] again (_next_x(batch, prev_states, i) for every k) -- and in a forecast; otherwise the loss step, whose
    next input takes forcing[:, i + 1].  ``xring``: the network inputs' buffers, re-used in turn (forecast), or None: one per call
    (they are kept for the reverse sweep).  ``keep_saved``: one ``saved`` buffer per call, kept with x in r.xs / r.saveds; otherwise
    ONE buffer serves every call."""
    ncalls = r.T * r.K
    x_next = saved = None
    for c in range(ncalls):
        i, k, prev, sbs_prev, new, sbs_new = _schedule(r, c)
        x = x_next
        if x is None:
            x = xring[c % len(xring)] if xring else _new_x(r)
            _build_x(r, i, prev, sbs_prev, x)
        if saved is None or keep_saved:
            saved = torch.empty(r.saved_bytes, dtype=torch.uint8, device=x.device)
        _model_forward(r, x, saved)
        x_next = forcing_next = None
        if r.fuse_next and c + 1 < ncalls:
            x_next = xring[(c + 1) % len(xring)] if xring else _new_x(r)
            forcing_next = r.forcing[:, i if k < r.K - 1 else i + 1]
        step = _free_step if (k < r.K - 1 or r.loss is None) else _loss_step
        step(r, i, saved, prev, sbs_prev, new, sbs_new, x_next, forcing_next)
        if keep_saved:
            r.xs.append(x)
            r.saveds.append(saved)


def native_forecast(model, lm, batch, std, mean, K):
    """Forward-only native forecast (phase "inference", lightning.py:565-662 with ``inference``): T * K model calls, every one a
    free step without border forcing (:627) -- no autograd node, one ``saved`` buffer for all calls, states written straight into
    the (B,T,H,W,F) result (intermediary states of K >= 2 through two scratch buffers).  T comes from the forcing tensor
    (``batch.outputs`` is None).  T_in >= 2: the window buffer of the training rollout with p4c_build_x per call.  Returns None
    where ``native_rollout`` does (channel mismatch; padded grids unless ``padded_grid_is_native``: those run behind the window, with
    p4c_build_x_win per call and p4c_ar_update_next_win as the free step)."""
    inputs, forcing = batch.inputs.tensor, batch.forcing.tensor
    if forcing.dim() != 5:
        return None
    B, T_in, H, W, F = inputs.shape
    T = forcing.shape[1]
    statics = lm.grid_static_features[: batch.batch_size]
    mask_on_nan = int(bool(lm.mask_on_nan))
    channels = T_in * F + statics.shape[-1] + forcing.shape[-1] + mask_on_nan
    if channels != model.in_channels or F > model.out_channels or (K > 1 and T_in > 1):
        return None
    padding = model.padding_for(H, W)
    if any(padding) and not padded_grid_is_native(padding, model._settings.autopad_enabled, T_in, K, channels, model.in_channels):
        return None
    L.require_cuda(inputs, forcing)
    dev = inputs.device
    with torch.no_grad():
        model._running = model._running_stats(dev)
        training = model.training
        if training and model._settings.norm == "batch":
            torch._foreach_add_([nb.num_batches_tracked for nb in model._norms], T * K)
        r = _rollout_context(model, inputs.float().contiguous(), forcing.float().contiguous(), statics, std, mean, T, K, mask_on_nan,
                             training, node=False)
        _prepare_weights(r)
        _state_slots(r, window=not r.feed)
        r.inter = [torch.empty(B, H, W, F, dtype=torch.float32, device=dev) for _ in range(min(2, K - 1))]
        r.y = None if r.fused_tail else torch.empty(B, r.Hn, r.Wn, NF, dtype=r.adt, device=dev)
        _run_schedule(r, [_new_x(r) for _ in range(2 if r.fuse_next else 1)], keep_saved=False)
        return r.pred if r.feed else r.pred.contiguous()


class _NativeRolloutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, lm, inputs, forcing, outputs, statics, std, mean, border_flat, interior_flat, force_border,
                weights, num_interior, kind, mask_mode, training, keep_saved, K, *params):
        L.require_cuda(inputs, forcing, outputs)
        dev = inputs.device
        B, T = outputs.shape[0], outputs.shape[1]
        outputs = outputs.float().contiguous()
        r = _rollout_context(model, inputs.float().contiguous(), forcing.float().contiguous(), statics, std, mean, T, K,
                             int(mask_mode == L.MASK_FROM_NAN), training, node=True)
        N, F, H, W = r.N, r.F, r.H, r.W
        r.outputs, r.sbs_out = outputs, T * N * F
        r.border, r.interior, r.force_border = border_flat, interior_flat, force_border
        r.weights, r.num_interior, r.kind, r.mask_mode = weights, num_interior, kind, mask_mode
        if r.mask_on_nan:
            r.count = torch.empty(1, dtype=torch.int32, device=dev)
            L.call("p4c_mask_all_zero_count", L.ptr(outputs), mask_mode, T * N * F, N * F, B, T, N, F, L.ptr(r.count), r.stream)
        _state_slots(r, window=True)
        r.loss = torch.empty(B, T, dtype=torch.float32, device=dev)
        r.ws = torch.empty(L.lib().p4c_loss_workspace_bytes(B, 1, N, 1) // 4, dtype=torch.float32, device=dev)
        r.y = torch.empty(B, r.Hn, r.Wn, NF, dtype=r.adt, device=dev)
        _prepare_weights(r)
        # bf16 flavour, training: the update kernel also saves the loss gradient of every element as bf16 rows and the backward reads
        # those instead of the new state and the target (480 -> 120 bytes per grid point; P4C_SAVE_LOSS_GRAD=0: recompute)
        r.save_lg = (keep_saved and r.adt == torch.bfloat16 and r.step_capable and mask_mode == L.MASK_NONE
                     and L.diag_switch("P4C_SAVE_LOSS_GRAD") != "0")
        r.lgrads = torch.empty(T, B, N, F, dtype=torch.bfloat16, device=dev) if r.save_lg else None
        r.inter = [torch.empty(B, H, W, F, dtype=torch.float32, device=dev) for _ in range(min(2, K - 1))]
        # only activations (xs / saveds) are kept per call for the reverse sweep
        _run_schedule(r, None, keep_saved)
        loss = r.loss
        r.release_forward()
        ctx.r = r
        ctx.set_materialize_grads(False)
        return r.states[:, r.T_in:], loss   # (a view of its own: the context must not hold the node's output)

    @staticmethod
    def backward(ctx, g_pred, g_loss):
        r = ctx.r
        model, desc = r.model, r.desc
        dev = r.states.device
        stream = L.stream(dev)
        flat = model._flat_params()
        _, scratch = model._workspaces(desc, dev)
        target = model._flat_grad_target()
        new = lambda c: torch.empty(r.B, r.Hn, r.Wn, c, dtype=r.adt, device=dev)   # noqa: E731  (network side: the padded grid)
        # the scratch workspace may have served another call since forward: prepare again (one launch per sweep)
        w = SimpleNamespace(stream=stream, flat=flat, scratch=scratch, target=target,
                            gflat=target if target is not None else torch.zeros_like(flat), dy=new(NF),
                            dx=new(NF) if r.T_in == 1 else None,
                            dprev=torch.empty(r.B, r.H, r.W, r.F, dtype=torch.float32, device=dev),
                            gl=g_loss.contiguous().float() if g_loss is not None else None)
        L.call("p4c_halfunet_prepare_weights", ctypes.byref(desc), L.ptr(flat), L.ptr(scratch), stream)
        w.desc0 = HalfUNetDesc.from_buffer_copy(desc)
        w.desc0.dx_channels = 0  # the input state of step 0 is data: no gradient needed, skip that conv
        # Weight gradients run on the library's side stream.  Their join is deferred over the whole reverse sweep: the
        # full-resolution ones left over at the end of AR step i's backward then run beside the HBM-bound head of step i-1's
        # chain instead of alone (P4C_DEFER_JOIN=0: join after every step, the round-2 behaviour).  xs / saveds stay referenced
        # until the join in _finish_sweep -- the side stream reads them.
        w.defer = defer = r.T * r.K > 1 and L.diag_switch("P4C_DEFER_JOIN") != "0"
        if defer:
            L.call("p4c_side_stream_defer", 1)
        ok = False
        try:
            (_sweep_window if r.T_in > 1 else _sweep)(r, w, g_pred)
            out = _finish_sweep(r, w)
            ok = True
            return out
        finally:
            if defer:
                L.call("p4c_side_stream_defer", 0)
                if not ok:
                    # the sweep raised between two calls: weight gradients already on the side stream still read xs / saveds / dy,
                    # which the unwinding is about to release to the allocator -- make the caller's stream (the one the allocator
                    # orders re-use on) wait for them first.  (The join itself must not mask the original error.)
                    try:
                        L.call("p4c_side_stream_join", stream)
                    except Exception:  # noqa: BLE001
                        pass


# the gradient tuple: one None per argument of forward ahead of the parameters
_N_INPUTS = _NativeRolloutFn.forward.__code__.co_argcount - 1


def _step_backward(r, w, i, free, g_next, g_next2, dprev):
    """Adjoint of one AR step: dy (and dprev, unless NULL) from the gradients arriving at its new state (g_next fp32 state layout,
    g_next2 rows of the network's input gradient) -- of a free step (it reads nothing of the forward), from the saved loss gradients,
    or from the new state and the target."""
    state_sz = r.N * r.F
    grads = (L.ptr(g_next), state_sz, L.ptr(g_next2), r.acode, NF)
    out = (L.ptr(w.dy), r.acode, NF, L.ptr(dprev), state_sz, r.B, r.N, r.F, 1.0, w.stream)
    if free:
        L.call("p4c_ar_update_next_bwd", *grads, L.ptr(r.std), L.ptr(r.interior if r.force_border else None), int(r.force_border), *out)
        return
    gloss = (L.ptr(w.gl[:, i]) if w.gl is not None else None, r.T)
    loss = (L.ptr(r.std), L.ptr(r.interior), int(r.force_border), L.ptr(r.weights), r.num_interior, L.ptr(r.count), r.kind, r.mask_mode)
    recompute = (L.ptr(r.pred[:, i]), r.sbs_state, L.ptr(r.outputs[:, i]), r.sbs_out)
    if r.window:   # dx read and dy written through the window: every element of dy, zeros outside
        L.call("p4c_ar_update_loss_bwd_win", *grads, *gloss, *recompute, *loss, *out[:-1], *r.win_args, w.stream)
    elif r.lgrads is not None:
        L.call("p4c_ar_update_loss_bwd_saved", *grads, *gloss, L.ptr(r.lgrads[i]), state_sz, *loss, *out)
    else:
        L.call("p4c_ar_update_loss_bwd", *grads, *gloss, *recompute, *loss, *out)


def _model_backward(r, w, c, dx):
    """Backward plan of model call c (call 0's input is data: no input gradient); releases the call's activations as soon as it is
    enqueued unless the side stream's join is deferred."""
    L.call("p4c_halfunet_backward", ctypes.byref(r.desc if c > 0 else w.desc0), L.ptr(r.xs[c]), L.ptr(w.flat), L.ptr(w.dy),
           L.ptr(dx) if c > 0 else None, L.ptr(w.gflat), L.ptr(r.saveds[c]), L.ptr(w.scratch), int(r.training), w.stream)
    if not w.defer:
        r.xs[c] = None
        r.saveds[c] = None


def _finish_sweep(r, w):
    if w.defer:
        L.call("p4c_side_stream_join", w.stream)
        for c in range(len(r.xs)):
            r.xs[c] = None
            r.saveds[c] = None
    if w.target is not None:  # already accumulated into param.grad
        return (None,) * (_N_INPUTS + len(r.model._param_slices))
    return (None,) * _N_INPUTS + tuple(w.gflat[o : o + n].view(s) for (o, n, s) in r.model._param_slices)


def _sweep(r, w, g_pred):
    """Reverse sweep with one input state: all T * K model calls in reverse; call c = i * K + k is a free step for k < K - 1 (no loss
    gradient, no prediction slot, nothing saved)."""
    dprev, K = w.dprev, r.K
    have_next = False
    for c in range(r.T * K - 1, -1, -1):
        i, k = divmod(c, K)
        g_next = dprev if have_next else None
        if g_pred is not None and k == K - 1:  # somebody differentiates through the prediction itself: add its slice
            if g_next is None:
                dprev.copy_(g_pred[:, i])
            else:
                dprev.add_(g_pred[:, i])
            g_next = dprev
        _step_backward(r, w, i, k < K - 1, g_next, w.dx if have_next else None, dprev if c > 0 else None)
        _model_backward(r, w, c, w.dx)
        have_next = True


def _sweep_window(r, w, g_pred):
    """Reverse sweep of a rollout with T_in >= 2 input states.  State slot s = i + T_in (the new state of step i) collects, summed
    in one launch (p4c_sum_state_grads) before step i's update backward: its prediction's gradient, the residual path of step i+1
    (whose previous state it is: dprev), and block s - k of the input gradient dx_k of every step k in i+1 .. i+T_in whose window
    holds it.  dx_k lives in a ring of T_in + 1 buffers (written at step k, last read at step k - T_in).  Step 0's window is all
    input data: no data gradient there."""
    B, T, T_in, H, W, N, F = r.B, r.T, r.T_in, r.H, r.W, r.N, r.F
    dev = r.states.device
    dxw = NF * ((r.desc.dx_channels + NF - 1) // NF)
    nring = T_in + 1
    dxs = [torch.empty(B, H, W, dxw, dtype=r.adt, device=dev) for _ in range(min(nring, T))]
    gsum = torch.empty(B, H, W, F, dtype=torch.float32, device=dev)
    gp = g_pred.float().contiguous() if g_pred is not None else None
    srcs = (ctypes.c_void_p * 8)()
    sbs, scs, soff, sdt = (ctypes.c_int64 * 8)(), (ctypes.c_int * 8)(), (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
    for i in range(T - 1, -1, -1):
        n = 0
        parts = []
        if gp is not None:
            parts.append((gp[:, i], gp.stride(0), F, 0, L.F32))
        if i + 1 < T:
            parts.append((w.dprev, N * F, F, 0, L.F32))
        s = i + T_in
        for k in range(i + 1, min(i + T_in, T - 1) + 1):
            parts.append((dxs[k % nring], N * dxw, dxw, (s - k) * F, r.acode))
        for (t, bs, cs, off, dt) in parts:
            srcs[n], sbs[n], scs[n], soff[n], sdt[n] = t.data_ptr(), bs, cs, off, dt
            n += 1
        g_next = None
        if n:
            L.call("p4c_sum_state_grads", L.ptr(gsum), N * F, n, srcs, sbs, scs, soff, sdt, B, N, F, w.stream)
            g_next = gsum
        _step_backward(r, w, i, False, g_next, None, w.dprev if i > 0 else None)
        _model_backward(r, w, i, dxs[i % nring])
