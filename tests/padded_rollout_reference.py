"""
TEST INFRASTRUCTURE ONLY.  Float64 restatements of the four window kernels of csrc/rollout_win.hip -- the AR step of a rollout on an
auto-padded grid -- on top of tests/step_reference.py, and the launch arithmetic of those kernels restated in Python.  No product code.

Geometry: the NETWORK side (x, y, dy, dx) is rows of the padded grid, (B, Hp * Wp, channels); the STATE side (states, statics,
forcing, target, masks, dprev, g_next) is (B, H * W, ..).  State pixel (h, w) is network row (top + h) * Wp + left + w.  Outside that
window x and dy are +0.0 in every channel.  tests/test_padded_rollout_cpu.py proves these against oracle/rollout.py around
pad -> oracle/halfunet.py -> crop.
"""
import collections

import step_reference as S
import torch

Geom = collections.namedtuple("Geom", "H W Hp Wp top left")


def padding_for(H, W, multiple=16):
    """mfai's AutoPaddingModel: centred zero padding to the next multiple, the extra row / column at the end -> (top, bottom, left, right)"""
    dh, dw = (-H) % multiple, (-W) % multiple
    return dh // 2, dh - dh // 2, dw // 2, dw - dw // 2


def geom(H, W):
    top, bottom, left, right = padding_for(H, W)
    return Geom(H, W, H + top + bottom, W + left + right, top, left)


def window_rows(g):
    """(H * W,) network row of every state pixel"""
    h = torch.arange(g.H).repeat_interleave(g.W)
    w = torch.arange(g.W).repeat(g.H)
    return (g.top + h) * g.Wp + g.left + w


def crop_rows(rows, g):
    """(B, Hp * Wp, C) -> (B, H * W, C): differentiable gather through the window"""
    return rows[:, window_rows(g).to(rows.device)]


def pad_rows(state_rows, g):
    """(B, H * W, C) -> (B, Hp * Wp, C), +0.0 outside the window"""
    B, _, C = state_rows.shape
    out = torch.zeros(B, g.Hp * g.Wp, C, dtype=state_rows.dtype, device=state_rows.device)
    out[:, window_rows(g).to(state_rows.device)] = state_rows
    return out


def build_x(prev, statics, forcing, g, c_pad=None, out_dtype=torch.float32, mask_on_nan=False):
    """p4c_build_x_win: prev (B, N, F), statics (B, N, Fs), forcing (B, N, Ff) -> (B, Hp * Wp, c_pad): step_reference.build_x's row
    inside the window, zeros (every channel, the NaN-mask channel included) outside"""
    return pad_rows(S.build_x(prev.unsqueeze(1), statics, forcing, c_pad, out_dtype, mask_on_nan), g)


def fused_step(prev, y, target, std, mean, border_mask, interior_mask, weights, g, **kw):
    """p4c_ar_update_loss_fwd_win (loss=False: p4c_ar_update_next_win): step_reference.fused_step on y (B, Hp * Wp, y_cs) read through
    the window.  ``y`` may require grad: the crop is part of the graph, so ``fused_step_grads`` returns dy on the padded grid."""
    return S.fused_step(prev, crop_rows(y, g), target, std, mean, border_mask, interior_mask, weights, **kw)


def fused_step_grads(out, y, prev, g, gloss=None, g_next=None, g_next2=None, **kw):
    """p4c_ar_update_loss_bwd_win: (dy (B, Hp * Wp, y_cs) -- zero outside the window and in channels >= F --, dprev (B, N, F)); g_next2
    are rows of the padded grid"""
    return S.fused_step_grads(out, y, prev, gloss=gloss, g_next=g_next, g_next2=None if g_next2 is None else crop_rows(g_next2, g), **kw)


def ar_update(prev, y, g, **kw):
    """the state update alone, y read through the window"""
    return S.ar_update(prev, crop_rows(y, g), **kw)


# ------------------------------------------------------------------------------------------------ routing
def routes_natively(padding, autopad_enabled, T_in, K, channels, in_channels):
    """what halfunet_rollout.padded_grid_is_native has to answer, restated"""
    if not any(padding):
        return False
    return bool(autopad_enabled) and T_in == 1 and K == 1 and channels == in_channels


# ------------------------------------------------------------------------------------------------ launch arithmetic
def blocks_per_sample(pixels, PP, B, cus):
    """rollout_win.hip blocks_per_sample: the rule of losses.hip's loss_blocks"""
    return S.loss_blocks(pixels, PP, B, cus)


def win_trips(pixels, lanes_per_pixel, B, cus):
    """passes of the busiest wave of a window kernel: ``pixels`` = H * W for the forward steps, Hp * Wp for build_x and the backward;
    ``lanes_per_pixel`` = pow2_ge64 of the quads (16-byte kernels) or channels (scalar kernels) of a row"""
    PP = 64 // lanes_per_pixel
    return S.trips(pixels, PP, S.WAVES_PER_BLOCK * blocks_per_sample(pixels, PP, B, cus))


def two_trip_side(lanes_per_pixel, B, cus):
    """smallest H = W (not a multiple of 16) whose H * W state pixels take a wave of a window kernel through a second pass"""
    PP = 64 // lanes_per_pixel
    cap = min(max(-(-cus * 8 // B), 1), S.LOSS_MAX_BLOCKS)
    side = int((cap * S.WAVES_PER_BLOCK * PP) ** 0.5) + 1
    while side % 16 == 0 or win_trips(side * side, lanes_per_pixel, B, cus) < 2:
        side += 1
    return side
