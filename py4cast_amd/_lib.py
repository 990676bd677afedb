"""
ctypes binding of ``libpy4cast_hip.so`` (C ABI: ``include/py4cast_hip.h``).

The product path has NO CPU fallback: if the shared library is missing or a symbol is
absent, import-time / call-time errors are raised.  Build it with
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C py4cast_amd/csrc``.
"""

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p
from typing import List, Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("P4C_LIB_PATH") or os.path.join(_HERE, "libpy4cast_hip.so")  # override: diagnostic builds

F32, BF16 = 0, 1
PROF_CONV3X3_C64, PROF_WGRAD3X3_C64, PROF_CONV3X3_C64_BWD = 1, 2, 4
LOSS_MSE, LOSS_L1 = 0, 1
MASK_NONE, MASK_FROM_NAN, MASK_F32, MASK_U8 = 0, 1, 2, 3
EVAL_MAP_NONE = -1
OK, ERR_INVALID, ERR_LAUNCH, ERR_RUNTIME, ERR_UNSUPPORTED = 0, -1, -2, -3, -4   # the return codes of every entry point

P = c_void_p
I = c_int
L = c_int64
F = c_float

# name -> argtypes (restype is int unless noted).  Mirrors include/py4cast_hip.h one to one.
SIGNATURES = {
    "p4c_build_x": [P, L, L, P, L, P, L, P, I, I, I, I, L, I, I, I, I, I, P],
    "p4c_build_x_bwd": [P, I, I, P, I, I, L, I, P],
    "p4c_sum_state_grads": [P, L, I, P, P, P, P, P, I, L, I, P],
    "p4c_build_x_masked": [P, L, L, P, L, P, L, P, I, I, I, I, L, I, I, I, I, I, P, I, I, I, I, P],
    "p4c_build_x_bwd_masked": [P, I, I, P, I, I, L, I, P, I, I, I, I, P],
    "p4c_ar_update_fwd": [P, L, P, I, I, P, L, P, P, P, P, P, L, I, L, I, F, I, P],
    "p4c_ar_update_bwd": [P, L, P, P, P, I, I, P, L, I, L, I, F, P],
    "p4c_mask_all_zero_count": [P, I, L, L, I, I, L, I, P, P],
    "p4c_weighted_loss_fwd": [P, L, L, P, L, L, P, I, P, P, F, P, I, P, P, I, I, L, I, P],
    "p4c_weighted_loss_map": [P, L, L, P, L, L, P, I, P, I, P, I, I, L, I, P],
    "p4c_weighted_loss_bwd": [P, P, L, L, P, L, L, P, I, P, P, F, P, I, P, L, L, I, I, L, I, P],
    "p4c_scaled_loss_fwd": [P, L, L, P, L, L, P, I, P, P, F, P, I, P, P, I, I, L, I, P],
    "p4c_acc_sums": [P, L, L, P, L, L, P, I, P, P, P, I, I, L, I, P],
    # pred, bs, ts, target, bs, ts, mask, mode, interior, num_interior, std, weights, map_kind, map_acc, accumulate, scores, count, ws,
    # B, T, N, F, stream
    "p4c_eval_sums": [P, L, L, P, L, L, P, I, P, F, P, P, I, P, I, P, P, P, I, I, L, I, P],
    "p4c_psd": [P, L, P, L, P, L, I, P, P, I, P, P, I, I, I, I, P],
    "p4c_unnormalize": [P, P, P, P, L, I, P],
    "p4c_unnormalize_planes": [P, P, P, P, L, L, I, P],
    "p4c_adamw_step": [P, P, P, P, L, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, L, P],
    "p4c_nan_moments": [P, P, L, P, P, I, L, I, P],
    "p4c_pack_standardize": [P, L, P, P, P, L, I, P],
    "p4c_build_forcing": [P, L, P, P, P, P, P, P, P, I, I, L, I, P],
    # feats, taps, out, B, T, H_sub, W_sub, F, stream
    "p4c_regrid_pack": [P, P, P, I, I, I, I, I, P],
    # feats (device), out, dtype, vec, B, T, H, W, F, stream
    "p4c_pack_convert": [P, P, I, I, I, I, I, I, I, P],
    # src, plane_stride, pitch, row0, col0, dst, planes, n, m, row_index, col_index, row_w, ry, col_w, rx, stream
    "p4c_regrid_blur": [P, L, I, I, I, P, I, I, I, P, P, P, I, P, I, P],
    # pred, bs, ts, target, bs, ts, mask, mode, std, mean, features, planes, vrange, ws, n, T, N, F, K, stream
    "p4c_map_planes": [P, L, L, P, L, L, P, I, P, P, P, P, P, P, I, I, L, I, I, P],
    # planes, vrange, lut, interior, frames, n, T, K, H, W, stream
    "p4c_map_render": [P, P, P, P, P, I, I, I, I, I, P],
    # pred, bs, ts, samples (host), std, mean, features, display, auto_range, frames, vrange, ws, B, n, T, H, W, F, K, stream
    "p4c_forecast_frames": [P, L, L, P, P, P, P, P, I, P, P, P, I, I, I, I, I, I, I, P],
    # pred, bs, ts, samples (host), std, mean, features, spec (host), flip_rows, params, packed, pitch, ws, B, n, T, H, W, F, K, stream
    "p4c_grib_pack": [P, L, L, P, P, P, P, P, I, P, P, L, P, I, I, I, I, I, I, I, P],
    # pred, bs, ts, samples (host), std, mean, features, spec (host, K x 3), flip_rows, params, out, out_bytes, ws, B, n, T, H, W, F, K, stream
    "p4c_grib_pack_complex": [P, L, L, P, P, P, P, P, I, P, P, L, P, I, I, I, I, I, I, I, P],
    # bytes, nbytes, fields (device), fields (host), nfields, planes, ws, stream
    "p4c_grib_unpack": [P, L, P, P, I, P, P, P],
    # bytes, nbytes, fields (device), fields (host), nfields, planes, status, ws, stream
    "p4c_grib_unpack_complex": [P, L, P, P, I, P, P, P, P],
    # bytes, nbytes, fields (device), fields (host), out, B, T, H, W, F, stream
    "p4c_grib_window_pack": [P, L, P, P, P, I, I, I, I, I, P],
    "p4c_ar_update_loss_fwd": [P, L, P, I, I, P, L, P, P, P, P, P, L, P, F, P, I, I, P, L, P, I, L, I, F, P],
    "p4c_ar_update_loss_fwd_next": [P, L, P, I, I, P, L, P, P, P, P, P, L, P, F, P, I, I, P, L, P, I, L, I, F,
                                    P, I, P, L, I, P, L, I, P],
    "p4c_ar_update_loss_bwd": [P, L, P, I, I, P, L, P, L, P, L, P, P, I, P, F, P, I, I, P, I, I, P, L, I, L, I, F, P],
    # a, a_scale, a_shift, wout, cout | prev, prev_bs, target, tgt_bs, std, mean, border, interior, new_state, new_bs, weights, num_interior,
    # masked_count, kind, loss_out, loss_stride, workspace, B, N, F, keep_prev | x_next, c_pad, statics, statics_bs, Fs, forcing, forcing_bs, Ff,
    # lgrad, lgrad_bs, stream
    "p4c_out_conv_update_loss_fwd": [P, P, P, P, I, P, L, P, L, P, P, P, P, P, L, P, F, P, I, P, L, P, I, L, I, F,
                                     P, I, P, L, I, P, L, I, P, L, P],
    "p4c_ar_update_loss_fwd_next_saved": [P, L, P, I, I, P, L, P, P, P, P, P, L, P, F, P, I, I, P, L, P, I, L, I, F,
                                          P, I, P, L, I, P, L, I, P, L, P],
    "p4c_ar_update_loss_bwd_saved": [P, L, P, I, I, P, L, P, L, P, P, I, P, F, P, I, I, P, I, I, P, L, I, L, I, F, P],
    # the free step (no loss term): prev, prev_bs, y, y_dtype, y_cs, target, tgt_bs, std, mean, border, interior, new_state, new_bs,
    # nan_to_num, B, N, F, keep_prev | x_next, c_pad, statics, statics_bs, Fs, forcing, forcing_bs, Ff, stream
    "p4c_ar_update_next": [P, L, P, I, I, P, L, P, P, P, P, P, L, I, I, L, I, F, P, I, P, L, I, P, L, I, P],
    # a, a_scale, a_shift, wout, cout | prev, prev_bs, target, tgt_bs, std, mean, border, interior, new_state, new_bs, B, N, F, keep_prev |
    # x_next, c_pad, statics, statics_bs, Fs, forcing, forcing_bs, Ff, stream
    "p4c_out_conv_update_fwd": [P, P, P, P, I, P, L, P, L, P, P, P, P, P, L, I, L, I, F, P, I, P, L, I, P, L, I, P],
    # g_next, g_next_bs, g_next2, g2_dtype, g2_cs, std, interior, force_border, dy, dy_dtype, y_cs, dprev, dprev_bs, B, N, F, keep_prev, stream
    "p4c_ar_update_next_bwd": [P, L, P, I, I, P, P, I, P, I, I, P, L, I, L, I, F, P],
    # the AR step on an auto-padded grid (csrc/rollout_win.hip): the arguments of p4c_build_x / p4c_ar_update_loss_fwd / p4c_ar_update_next
    # (without a next input) / p4c_ar_update_loss_bwd, then the window H, W, Hp, Wp, top, left, then the stream
    "p4c_build_x_win": [P, L, L, P, L, P, L, P, I, I, I, I, L, I, I, I, I, I, I, I, I, I, I, I, P],
    "p4c_ar_update_loss_fwd_win": [P, L, P, I, I, P, L, P, P, P, P, P, L, P, F, P, I, I, P, L, P, I, L, I, F, I, I, I, I, I, I, P],
    "p4c_ar_update_next_win": [P, L, P, I, I, P, L, P, P, P, P, P, L, I, I, L, I, F, I, I, I, I, I, I, P],
    "p4c_ar_update_loss_bwd_win": [P, L, P, I, I, P, L, P, L, P, L, P, P, I, P, F, P, I, I, P, I, I, P, L, I, L, I, F, I, I, I, I, I, I, P],
}
OTHER = {
    "p4c_version": ([], c_int),
    "p4c_graph_replace_memsets": ([P, ctypes.POINTER(c_int), ctypes.POINTER(c_int)], c_int),
    "p4c_last_error": ([], c_char_p),
    "p4c_num_cus": ([], c_int),
    "p4c_loss_workspace_bytes": ([I, I, L, I], c_size_t),
    "p4c_psd_workspace_bytes": ([I, I, I, I], c_size_t),
    "p4c_eval_sums_workspace_bytes": ([I, I, L, I], c_size_t),
    "p4c_map_planes_workspace_bytes": ([I, I, L, I], c_size_t),
    "p4c_pack_convert_rows": ([I], c_int),
    "p4c_pack_convert_max_blocks": ([], c_int),
    "p4c_map_tile": ([], c_int),
    "p4c_map_max_blocks": ([], c_int),
    "p4c_map_gap": ([], c_int),
    "p4c_map_render_pixels": ([], c_int),
    "p4c_map_render_max_blocks": ([], c_int),
    "p4c_forecast_frames_workspace_bytes": ([I, I, L, I], c_size_t),
    "p4c_forecast_tile": ([], c_int),
    "p4c_forecast_max_blocks": ([], c_int),
    "p4c_forecast_max_features": ([], c_int),
    "p4c_forecast_max_samples": ([], c_int),
    "p4c_forecast_frames_dense": ([I, I], c_int),
    "p4c_grib_pack_workspace_bytes": ([I, I, L, I], c_size_t),
    "p4c_grib_tile": ([], c_int),
    "p4c_grib_max_blocks": ([], c_int),
    "p4c_grib_max_features": ([], c_int),
    "p4c_grib_max_samples": ([], c_int),
    "p4c_grib_pack_dense": ([I, I], c_int),
    "p4c_grib_pack_complex_group": ([], c_int),
    "p4c_grib_pack_complex_params": ([], c_int),
    "p4c_grib_pack_complex_scan_threads": ([], c_int),
    "p4c_grib_pack_complex_capacity": ([I, I, L, P, I], c_int64),
    "p4c_grib_pack_complex_workspace_bytes": ([I, I, L, I, I], c_size_t),
    "p4c_grib_unpack_tile": ([], c_int),
    "p4c_grib_unpack_max_blocks": ([], c_int),
    "p4c_grib_unpack_fast": ([I, I], c_int),
    "p4c_grib_unpack_workspace_bytes": ([L], c_size_t),
    "p4c_grib_complex_tile": ([], c_int),
    "p4c_grib_complex_chunk": ([], c_int),
    "p4c_grib_complex_max_blocks": ([], c_int),
    "p4c_grib_unpack_complex_workspace_bytes": ([L, L, I], c_size_t),
    "p4c_grib_window_max_features": ([], c_int),
    "p4c_set_side_stream": ([P, P, I], c_int),
    "p4c_ghost_dw_fwd": ([P, P, P, I, I, I, I, P], c_int),
    "p4c_ghost_dw_bwd_data": ([P, P, P, I, I, I, I, P], c_int),
    "p4c_ghost_dw_wgrad_blocks": ([I, I, I], c_int),
    "p4c_ghost_dw_wgrad": ([P, P, P, I, I, I, I, P], c_int),
    "p4c_ghost_tail_blocks": ([I, I, I], c_int),
    "p4c_ghost_tail_fwd": ([P, I, P, P, I, P, I, I, I, I, P], c_int),
    "p4c_ghost_tail_bwd_blocks": ([I, I, I], c_int),
    "p4c_ghost_tail_bwd": ([P, P, I, P, P, I, P, I, I, I, I, P], c_int),
    "p4c_halfunet_merge_fwd": ([P, P, P, P, P, P, I, I, I, I, I, P], c_int),
    "p4c_halfunet_merge_bwd": ([P, P, P, P, P, P, P, P, P, I, I, I, I, I, P], c_int),
    "p4c_inorm_blocks": ([L, I], c_int),
    "p4c_inorm_reduce": ([P, P, P, P, P, F, P, I, I, L, I, P], c_int),
    "p4c_inorm_apply": ([P, P, P, P, P, P, P, P, P, P, F, P, P, I, I, L, I, P], c_int),
    "p4c_inorm_apply_mul": ([P, P, P, P, P, P, P, P, P, P, F, P, P, I, I, L, I, P, L, F, P], c_int),
    "p4c_inorm_reduce_mul": ([P, P, P, P, P, F, P, I, I, L, I, P, L, F, P], c_int),
    "p4c_inorm_finalize_fwd": ([P, I, I, L, I, I, P, P, F, P, P, P, P, P], c_int),
    "p4c_inorm_reduce_finalize_fwd": ([P, P, P, P, P, F, P, P, P, P, I, I, L, I, P], c_int),
    "p4c_inorm_reduce_finalize_bwd": ([P, P, P, P, P, F, P, P, P, P, P, P, I, I, L, I, P], c_int),
    "p4c_inorm_finalize_bwd": ([P, I, I, L, I, I, P, P, P, P, P, P, P], c_int),
    "p4c_ts_gram_splits": ([L], c_int),
    "p4c_ts_gram": ([P, I, L, L, L, P, I, L, L, L, P, I, I, L, I, I, P], c_int),
    "p4c_ts_apply_wide_ok": ([I, I, I, I], c_int),
    "p4c_ts_gram_wide_ok": ([I, I, I, I], c_int),
    "p4c_ts_apply_softmax": ([P, L, L, L, P, L, P, L, L, L, I, I, L, I, I, I, P, L, L, L, P], c_int),
    "p4c_ts_apply": ([P, I, L, L, L, P, L, P, I, L, L, L, I, I, L, I, I, I, P], c_int),
    "p4c_ts_apply_mt": ([P, I, L, L, L, P, L, P, I, L, L, L, I, I, L, I, I, I, P], c_int),
    "p4c_ts_apply_mt_ok": ([P, I, L, L, L, P, L, P, I, L, L, L, I, I], c_int),
    "p4c_epa_small_fwd": ([P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, P], c_int),
    "p4c_epa_small_bwd": ([P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, P], c_int),
    "p4c_ts_gram_norms": ([P, I, L, L, L, P, I, L, L, L, P, I, I, L, I, I, P], c_int),
    "p4c_ts_reduce_splits": ([P, I, I, I, I, I, P, P, P, I, I, P], c_int),
    "p4c_ts_reduce_transpose": ([P, I, L, I, P, I, P], c_int),
    "p4c_ts_colsums": ([I, P, P, P, P, P], c_int),
    "p4c_ts_merge_published": ([P, P, I, L, I, I, I, P], c_int),
    "p4c_prof_enable": ([I, I], c_int),
    "p4c_prof_filter": ([L], c_int),
    "p4c_prof_collect": ([I, L, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_double)], c_int),
}

_lib = None

# bumped whenever a kernel updates parameters through raw pointers (FlatAdamW): caches of re-laid parameters key on it as well
# as on tensor._version
PARAM_EPOCH = [0]


def invalidate_param_caches():
    """Tell the per-parameter caches (bf16 casts, re-laid weight images) that parameter storage was written behind autograd's
    back: ``p.data.copy_`` (an EMA / SWA swap), a third-party optimizer that writes through ``.data``, a collective into
    ``p.data``.  ``tensor._version`` does not move for such writes; FlatAdamW, FlatDDP.broadcast_parameters and
    FlatDDP.all_gather_params call this themselves ("Parameter caches")."""
    PARAM_EPOCH[0] += 1


# Gradients written IN PLACE (ops_gemm.GRADS_IN_PLACE, graphlam.GRADS_IN_PLACE: a reduction kernel adds dW into the parameter's .grad
# buffer, autograd gets None) pass no AccumulateGrad node, so no per-parameter hook fires for them.  A gradient exchange that wants to
# start inside the backward (trainer.FlatDDP(overlap=True)) listens here instead:
#   * grad_sink_taken(view)  -- a forward pass took `view` (a region of some parameter's .grad) as the destination of a later backward;
#   * grad_written(*views)   -- the kernels that ADD into these regions have just been enqueued on the current stream (called from
#                               inside the backward pass, after the launch: a stream that waits for the current one sees the sums).
GRAD_SINK_LISTENERS = []


def grad_sink_taken(view):
    for listener in GRAD_SINK_LISTENERS:
        listener.sink_taken(view)


def grad_written(*views):
    if GRAD_SINK_LISTENERS:
        for listener in GRAD_SINK_LISTENERS:
            listener.written(views)


class GradQueue:
    """Deferred reduction of the gradient partials of ONE backward pass (include/py4cast_hip.h: the ``defer`` argument of
    p4c_gemm_tn, p4c_row_mlp_bwd_accumulate and p4c_node_proj_wgrad; p4c_grad_reduce_flush).  The queued reductions run 32 per launch
    when the autograd engine finishes the pass (``queue_callback``); ``keep`` (the partials' workspace) stays alive until then.
    Outside a backward pass (no graph task) nothing is deferred."""

    enabled = True          # False: every call reduces at once (the A/B reference of tests/test_nodeproj_gpu.py, test_gemm_gpu.py)
    _task = -1
    _keep: List[torch.Tensor] = []
    _views: List[torch.Tensor] = []      # the .grad regions the queued reductions will add into (told to grad_written at the flush)
    _stream = None

    @classmethod
    def join(cls, keep: torch.Tensor, start: bool) -> bool:
        """The ``defer`` flag of the call about to be made: True when this backward pass is deferring its reductions -- or starts to,
        with ``start`` -- and then ``keep`` is held until the flush."""
        task = torch._C._current_graph_task_id()
        if cls._task >= 0 and cls._task != task:   # a pass that died before its callback ran: its queued jobs are void
            lib().p4c_grad_reduce_drop()
            cls._task, cls._keep, cls._views, cls._stream = -1, [], [], None
        if not cls.enabled or task < 0:
            return False
        if cls._task != task:
            if not start:
                return False
            cls._task, cls._stream = task, torch.cuda.current_stream(keep.device)
            torch.autograd.Variable._execution_engine.queue_callback(cls.flush)
        cls._keep.append(keep)
        return True

    @classmethod
    def wrote(cls, views, deferred: bool) -> None:
        """After the launch that produced the partials: ``views`` (regions of parameters' .grad) receive their sums when the queue is
        flushed (``deferred``, what ``join`` returned) or have just received them."""
        if not GRAD_SINK_LISTENERS:
            return
        views = [v for v in views if v is not None]
        if deferred:
            cls._views.extend(views)
        else:
            grad_written(*views)

    @classmethod
    def flush(cls) -> None:
        if cls._task < 0:
            return
        views = cls._views
        try:
            check(lib().p4c_grad_reduce_flush(c_void_p(cls._stream.cuda_stream)), "p4c_grad_reduce_flush")
        finally:
            cls._task, cls._keep, cls._views, cls._stream = -1, [], [], None
        if views:
            grad_written(*views)


# Values derived from the parameters (re-laid weight images, bf16 copies of weight blocks) are cached per parameter version in
# eager mode.  Inside a HIP-graph capture they must be produced by kernels of THAT graph (a replay has to see the current
# parameters), but once per capture is enough: the capturing code (trainer.GraphedTrainingStep) opens a scope, the ops keep what
# they derived in it -- which also keeps those tensors allocated, hence intact, until the capture ends.
CAPTURE_SCOPE = [None]


def _base(t):
    t = t._base if t._base is not None else t
    return getattr(t, "_p4c_owner", t)      # a rollout's per-step stand-in of a parameter (trainer.RolloutParamProxies): the parameter


def owner_refs(tensors):
    """Weak references to the tensors that own the storage of `tensors` (parameters, for slices of parameters).  A cache keyed by
    addresses and version counters alone can hit a DIFFERENT parameter that the allocator placed at a freed one's address."""
    import weakref

    return tuple(None if t is None else weakref.ref(_base(t)) for t in tensors)


def owners_alive(refs, tensors) -> bool:
    return all((r is None and t is None) or (r is not None and t is not None and r() is _base(t)) for r, t in zip(refs, tensors))


def capture_cache():
    """The dict of the capture in progress, or None (not capturing, or a capture nobody opened a scope for: derive every time)."""
    import torch

    if CAPTURE_SCOPE[0] is not None and torch.cuda.is_current_stream_capturing():
        return CAPTURE_SCOPE[0]
    return None


class P4CError(RuntimeError):
    pass


def _declare(lib, signatures, other):
    for name, argtypes in signatures.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: loud by design
        fn.argtypes = argtypes
        fn.restype = c_int
    for name, (argtypes, restype) in other.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype


def all_symbols():
    from . import _lib_model  # model-side signatures live next to their wrappers

    names = list(SIGNATURES) + list(OTHER) + list(_lib_model.SIGNATURES) + list(_lib_model.OTHER)
    return names


def lib():
    """Load (once) and return the ctypes handle.  Raises if the extension was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise P4CError(
                f"{LIB_PATH} not found: the HIP extension is not built. "
                "Run `python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)."
            )
        handle = ctypes.CDLL(LIB_PATH)
        _declare(handle, SIGNATURES, OTHER)
        from . import _lib_model

        _declare(handle, _lib_model.SIGNATURES, _lib_model.OTHER)
        _lib = handle
    return _lib


def kernel_sources_sha16() -> str:
    """sha256 (first 16 hex digits) over the kernel sources of this tree (csrc/*.hip, *.cpp, *.hpp, the C header): what a committed
    PMC traffic figure under profiles/ was measured on.  bench.py reports such a figure as `traffic` only when it matches the running
    tree; a changed kernel keeps the pointer to the file and a null number."""
    import glob
    import hashlib

    h = hashlib.sha256()
    root = os.path.join(_HERE, "csrc")
    files = sorted(glob.glob(os.path.join(root, "*.hip")) + glob.glob(os.path.join(root, "*.cpp")) + glob.glob(os.path.join(root, "*.hpp")))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "py4cast_hip.h"))
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def committed_traffic(names, key=None):
    """(value, source note) from the first of the profiles/ JSON files `names` that exists: the value only if the file records the
    kernel sources of THIS tree (kernel_sources_sha16), else None with a note that names the file as stale."""
    import json

    root = os.path.dirname(_HERE)
    for name in names:
        f = os.path.join(root, "profiles", name)
        if not os.path.exists(f):
            continue
        try:
            d = json.load(open(f))
        except (OSError, ValueError):
            continue
        sha = d.get("kernel_sources_sha16")
        val = d
        for k in (key or ()):
            val = val.get(k, {}) if isinstance(val, dict) else None
        if not isinstance(val, (int, float)):
            continue
        if sha == kernel_sources_sha16():
            return val, f"profiles/{name} (committed rocprofv3 --pmc passes on this tree's kernel sources, sha {sha})"
        return None, (f"profiles/{name} holds {val:.4g} B measured on other kernel sources (sha {sha}; this tree: "
                      f"{kernel_sources_sha16()}): not reported as this run's traffic")
    return None, None


DIAG_LIB_PATH = os.path.join(_HERE, "libpy4cast_hip_diag.so")
_diag = None


class use_diagnostic_library:
    """Context manager: route every call of this process to libpy4cast_hip_diag.so (``make -C py4cast_amd/csrc diag``) -- the same
    sources built with -DP4C_DIAG_BUILD, where the P4C_* environment switches that select an older kernel / another geometry are
    live.  The product library reads none of them.  For the A/B parity tests and tools/diagnostics only."""

    def __enter__(self):
        global _lib, _diag
        if not os.path.exists(DIAG_LIB_PATH):
            raise P4CError(f"{DIAG_LIB_PATH} not found: run `make -C py4cast_amd/csrc diag` (or __graft_entry__.build())")
        lib()
        if _diag is None:
            _diag = ctypes.CDLL(DIAG_LIB_PATH)
            _declare(_diag, SIGNATURES, OTHER)
            from . import _lib_model

            _declare(_diag, _lib_model.SIGNATURES, _lib_model.OTHER)
        self._saved = _lib
        _lib = _diag
        invalidate_param_caches()      # derived tensors of the other library's plans are not this one's
        return _diag

    def __exit__(self, *exc):
        global _lib
        _lib = self._saved
        invalidate_param_caches()
        return False


def diag_switch(name: str):
    """The value of a P4C_* ROUTE switch (an older kernel / a library route as the A/B reference of the native one), or None.  Like the C
    library's diag_env (csrc/common.hpp) these switches exist in DIAGNOSTIC mode only -- inside ``use_diagnostic_library()``, which the
    A/B parity tests (tests/conftest.py::diag_library) and tools/diagnostics enter: the product package reads no route switch from the
    environment, so a deployment cannot differ silently from the measured configuration.  The settings that ARE read from
    the environment are documented ones and bench.py echoes them (config.environment_settings): P4C_NO_AFFINITY, P4C_NO_TUNED_GEMMS,
    P4C_LIB_PATH."""
    if _diag is not None and _lib is _diag:
        return os.environ.get(name)
    return None


def environment_settings():
    """the documented environment settings in force (bench.py: config.environment_settings)"""
    return {k: os.environ[k] for k in ("P4C_NO_AFFINITY", "P4C_NO_TUNED_GEMMS", "P4C_LIB_PATH", "PYTORCH_TUNABLEOP_ENABLED", "MIOPEN_FIND_MODE")
            if k in os.environ}


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().p4c_last_error()
        raise P4CError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


# ---- optional per-entry-point timing with HIP events on the launch stream (bench.py roofline leg)
_TIMED = None


def enable_kernel_timing(names):
    """Record a HIP event pair around every call of the named entry points (None disables)."""
    global _TIMED
    _TIMED = None if names is None else {n: [] for n in names}


def kernel_times():
    """{name: (calls, avg_ms)} for the calls recorded since enable_kernel_timing (synchronises)."""
    out = {}
    if _TIMED:
        torch.cuda.synchronize()
        for n, evs in _TIMED.items():
            if evs:
                out[n] = (len(evs), sum(a.elapsed_time(b) for a, b, _ in evs) / len(evs))
    return out


def kernel_bytes():
    """{name: algorithmic HBM bytes summed over the recorded calls} for the entry points whose wrappers state them."""
    out = {}
    if _TIMED:
        for n, evs in _TIMED.items():
            if evs and all(nb is not None for _, _, nb in evs):
                out[n] = float(sum(nb for _, _, nb in evs))
    return out


def entry_point_roofline(ktimes):
    """bench.py's roofline object of a model that times its native entry points: the achieved HBM rate of the one that takes the most
    time -- the algorithmic bytes of its calls (stated by the wrappers next to each call, kernel_bytes()) over their HIP-event
    durations ``ktimes`` = kernel_times().  None when no timed entry point states its bytes."""
    nbytes = kernel_bytes()
    names = [k for k in ktimes if k in nbytes]
    if not names:
        return None
    name = max(names, key=lambda k: ktimes[k][0] * ktimes[k][1])
    calls, avg_ms = ktimes[name]
    gbs = nbytes[name] / (calls * avg_ms * 1e-3) / 1e9
    return {"bound": "hbm", "kernel": f"{name} (all launches)", "achieved": gbs, "peak": 8000.0, "unit": "GB/s",
            "frac": gbs / 8000.0, "traffic": None, "algorithmic_bytes_per_launch": nbytes[name] / calls,
            "avg_launch_ms": avg_ms, "launches": calls,
            "all": {k: {"calls": ktimes[k][0], "avg_ms": round(ktimes[k][1], 4),
                        "GBps": round(nbytes[k] / (ktimes[k][0] * ktimes[k][1] * 1e-3) / 1e9, 1)} for k in names}}


# bench.py's step-level roofline of the widened models: with WORK[0] a dict, every native call adds the algorithmic HBM bytes / matrix
# flops its wrapper states ({"bytes": .., "flops": .., "calls": .., "unstated": ..}); None = off (no cost on the product path)
WORK = [None]


def call(name: str, *args, alg_bytes=None, alg_flops=None):
    """alg_bytes / alg_flops: the call's algorithmic HBM bytes and matrix flops (roofline bookkeeping of bench.py; ignored unless
    timing / work counting is enabled)."""
    w = WORK[0]
    if w is not None:
        w["calls"] += 1
        if alg_bytes is None:
            w["unstated"] += 1
        else:
            w["bytes"] += alg_bytes
        if alg_flops:
            w["flops"] += alg_flops
    if _TIMED is not None and name in _TIMED:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()  # torch's current stream == the stream handed to the library
        check(getattr(lib(), name)(*args), name)
        b.record()
        _TIMED[name].append((a, b, alg_bytes))
        return
    check(getattr(lib(), name)(*args), name)


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else c_void_p(t.data_ptr())


def stream(device=None):
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    raise P4CError(f"unsupported dtype {dt}")


_TUNED_GEMMS_LOADED = [False]


def _load_tuned_gemms():
    """Once per process, at the first native call on a GPU tensor: hand the shipped GEMM selections (package __init__) to TunableOp."""
    _TUNED_GEMMS_LOADED[0] = True
    path = os.environ.get("P4C_TUNED_GEMMS_FILE")
    if not path:
        return
    try:
        import torch.cuda.tunable as tunable

        # lookup on, tuning and result files off: only the shipped selections are consulted, nothing is measured or written,
        # and a stray tunableop_results*.csv in the working directory is not picked up by a file-name default
        tunable.enable(True)
        tunable.tuning_enable(False)
        if hasattr(tunable, "write_file_on_exit"):
            tunable.write_file_on_exit(False)
        ok = tunable.read_file(path)
        if ok is False:   # validator lines of the file (torch / ROCm / hipBLASLt / GPU) do not match this stack
            import warnings

            warnings.warn("py4cast_amd: the shipped GEMM selections were rejected by TunableOp's validators (another torch / "
                          "ROCm / hipBLASLt build): library-default GEMM kernels are used")
    except Exception as exc:  # noqa: BLE001  (no TunableOp in this build / unreadable file: the library's default selection stays)
        import warnings

        warnings.warn(f"py4cast_amd: tuned GEMM selections not loaded ({type(exc).__name__}: {exc})")


def require_cuda(*tensors):
    if not _TUNED_GEMMS_LOADED[0] and any(t is not None and t.is_cuda for t in tensors):
        _load_tuned_gemms()
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise P4CError(
                "py4cast_amd kernels run on the GPU only (no CPU fallback); got a tensor on " + str(t.device)
            )
