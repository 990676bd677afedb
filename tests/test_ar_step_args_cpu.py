"""CPU checks of the AR step's host dispatch (csrc/losses.hip): calls the nine entry points refuse BEFORE any launch, each with its
return code and its p4c_last_error() text.  The pointer arguments are addresses inside one 16-byte aligned host buffer that no
call dereferences (every case returns from the argument checks or from the path selection).  The base call of every entry point
has F = 21 features on N = 5 grid points: N * F % 4 != 0, so neither the 16-byte nor the flat path applies.
Some messages name a sibling entry point: the shared implementations behind the wrappers do."""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -4
F32, BF16 = 0, 1
MASK_NONE, MASK_FROM_NAN, MASK_F32 = 0, 1, 2

_RAW = ctypes.create_string_buffer(4096 + 16)
BUF = (ctypes.addressof(_RAW) + 15) & ~15   # a non-null, 16-byte aligned address; never read or written

FWD = ("prev prev_bs y y_dtype y_cs target tgt_bs std mean border_mask interior_mask new_state new_bs weights num_interior "
       "masked_count kind mask_mode loss_out loss_stride workspace B N F keep_prev")
NEXT = "x_next c_pad statics statics_bs Fs forcing_next forcing_bs Ff"
OUT_CONV = "a a_scale a_shift wout cout prev prev_bs target tgt_bs std mean border_mask interior_mask new_state new_bs"
BWD_HEAD = "g_next g_next_bs g_next2 g2_dtype g2_cs"
BWD_TAIL = "dy dy_dtype y_cs dprev dprev_bs B N F keep_prev stream"
PARAMS = {
    "p4c_ar_update_loss_fwd": FWD + " stream",
    "p4c_ar_update_loss_fwd_next": FWD + " " + NEXT + " stream",
    "p4c_ar_update_loss_fwd_next_saved": FWD + " " + NEXT + " lgrad lgrad_bs stream",
    "p4c_ar_update_next": ("prev prev_bs y y_dtype y_cs target tgt_bs std mean border_mask interior_mask new_state new_bs "
                           "nan_to_num B N F keep_prev " + NEXT + " stream"),
    "p4c_out_conv_update_loss_fwd": (OUT_CONV + " weights num_interior masked_count kind loss_out loss_stride workspace B N F "
                                     "keep_prev " + NEXT + " lgrad lgrad_bs stream"),
    "p4c_out_conv_update_fwd": OUT_CONV + " B N F keep_prev " + NEXT + " stream",
    "p4c_ar_update_loss_bwd_saved": (BWD_HEAD + " gloss gloss_stride lgrad lgrad_bs std interior_mask force_border weights "
                                     "num_interior masked_count kind mask_mode " + BWD_TAIL),
    "p4c_ar_update_loss_bwd": (BWD_HEAD + " gloss gloss_stride new_state new_bs target tgt_bs std interior_mask force_border "
                               "weights num_interior masked_count kind mask_mode " + BWD_TAIL),
    "p4c_ar_update_next_bwd": BWD_HEAD + " std interior_mask force_border " + BWD_TAIL,
}
N, F, FS, FF, CPAD = 5, 21, 4, 5, 32
# a complete call of any of the nine: every pointer set (masked_count and stream NULL), one sample, bf16 rows of 64 channels
BASE = dict(
    prev=BUF, prev_bs=N * F, y=BUF, y_dtype=BF16, y_cs=64, target=BUF, tgt_bs=N * F, std=BUF, mean=BUF, border_mask=BUF,
    interior_mask=BUF, new_state=BUF, new_bs=N * F, weights=BUF, num_interior=float(N), masked_count=None, kind=0,
    mask_mode=MASK_NONE, loss_out=BUF, loss_stride=1, workspace=BUF, B=1, N=N, F=F, keep_prev=1.0, stream=None,
    x_next=BUF, c_pad=CPAD, statics=BUF, statics_bs=0, Fs=FS, forcing_next=BUF, forcing_bs=N * FF, Ff=FF, lgrad=BUF, lgrad_bs=N * F + 3,
    nan_to_num=0, a=BUF, a_scale=BUF, a_shift=BUF, wout=BUF, cout=32,
    g_next=BUF, g_next_bs=N * F, g_next2=BUF, g2_dtype=BF16, g2_cs=64, gloss=BUF, gloss_stride=1, force_border=1, dy=BUF,
    dy_dtype=BF16, dprev=BUF, dprev_bs=N * F)

NO_PATH_FWD = ("p4c_ar_update_loss_fwd_next: needs the 16-byte path (F % 4 == 0, F <= 64, aligned rows) or the flat path "
               "(F <= 64, N * F % 4 == 0, whole 16-byte slots per row, aligned rows, no NaN masks)")
NO_PATH_TAIL = ("p4c_out_conv_update_loss_fwd: F % 4 != 0 needs the flat path (F <= 64, N * F % 4 == 0, whole 16-byte slots per "
                "row of x_next, aligned rows)")

CASES = [
    # ---- p4c_ar_update_loss_fwd
    ("p4c_ar_update_loss_fwd", dict(y=None), INVALID, "p4c_ar_update_loss_fwd: null pointer"),
    ("p4c_ar_update_loss_fwd", dict(prev=None), INVALID, "p4c_ar_update_loss_fwd: prev is null but keep_prev != 0"),
    ("p4c_ar_update_loss_fwd", dict(mean=None), INVALID, "p4c_ar_update_loss_fwd: std and mean go together"),
    ("p4c_ar_update_loss_fwd", dict(mask_mode=MASK_F32), INVALID, "p4c_ar_update_loss_fwd: only MASK_NONE / MASK_FROM_NAN are fused"),
    ("p4c_ar_update_loss_fwd", dict(y_cs=20), INVALID, "p4c_ar_update_loss_fwd: bad F / y_cs"),
    ("p4c_ar_update_loss_fwd", dict(y_dtype=7), INVALID, "p4c_ar_update_loss_fwd: bad dtype 7"),
    # ---- p4c_ar_update_loss_fwd_next
    ("p4c_ar_update_loss_fwd_next", dict(statics=None), INVALID, "p4c_ar_update_loss_fwd_next: null pointer"),
    ("p4c_ar_update_loss_fwd_next", dict(c_pad=F + FS + FF - 1), INVALID, "p4c_ar_update_loss_fwd_next: c_pad must be >= F + Fs + Ff"),
    ("p4c_ar_update_loss_fwd_next", dict(mask_mode=MASK_FROM_NAN), INVALID,
     "p4c_ar_update_loss_fwd_next: the NaN-mask input channel is built by p4c_build_x"),
    ("p4c_ar_update_loss_fwd_next", dict(std=None), INVALID, "p4c_ar_update_loss_fwd: std and mean go together"),
    ("p4c_ar_update_loss_fwd_next", dict(), UNSUPPORTED, NO_PATH_FWD),
    # ---- p4c_ar_update_loss_fwd_next_saved
    ("p4c_ar_update_loss_fwd_next_saved", dict(lgrad=None), INVALID, "p4c_ar_update_loss_fwd_next_saved: lgrad rows must be 8-byte aligned"),
    ("p4c_ar_update_loss_fwd_next_saved", dict(lgrad_bs=N * F), INVALID,
     "p4c_ar_update_loss_fwd_next_saved: lgrad rows must be 8-byte aligned"),
    ("p4c_ar_update_loss_fwd_next_saved", dict(c_pad=F + FS + FF - 1), INVALID,
     "p4c_ar_update_loss_fwd_next_saved: c_pad must be >= F + Fs + Ff"),
    ("p4c_ar_update_loss_fwd_next_saved", dict(mask_mode=MASK_FROM_NAN), INVALID,
     "p4c_ar_update_loss_fwd_next_saved: the NaN-mask input channel is built by p4c_build_x"),
    ("p4c_ar_update_loss_fwd_next_saved", dict(x_next=None), UNSUPPORTED, NO_PATH_FWD),   # the last AR step: still no fast path
    # ---- p4c_ar_update_next
    ("p4c_ar_update_next", dict(B=0), INVALID, "p4c_ar_update_next: bad dims"),
    ("p4c_ar_update_next", dict(border_mask=None), INVALID, "p4c_ar_update_next: target and border_mask go together"),
    ("p4c_ar_update_next", dict(forcing_next=None), INVALID, "p4c_ar_update_next: null pointer"),
    ("p4c_ar_update_next", dict(c_pad=F + FS + FF - 1), INVALID, "p4c_ar_update_next: c_pad must be >= F + Fs + Ff"),
    ("p4c_ar_update_next", dict(nan_to_num=1), INVALID, "p4c_ar_update_next: the NaN-mask input channel is built by p4c_build_x"),
    ("p4c_ar_update_next", dict(interior_mask=None), INVALID,
     "p4c_ar_update_next: null pointer (border forcing needs border_mask, interior_mask and target)"),
    ("p4c_ar_update_next", dict(mean=None), INVALID, "p4c_ar_update_loss_fwd: std and mean go together"),
    ("p4c_ar_update_next", dict(), UNSUPPORTED, NO_PATH_FWD),
    # ---- p4c_out_conv_update_loss_fwd
    ("p4c_out_conv_update_loss_fwd", dict(wout=None), INVALID, "p4c_out_conv_update_loss_fwd: null pointer"),
    ("p4c_out_conv_update_loss_fwd", dict(mean=None), INVALID, "p4c_out_conv_update_loss_fwd: std and mean go together"),
    ("p4c_out_conv_update_loss_fwd", dict(cout=F - 1), INVALID, "p4c_out_conv_update_loss_fwd: needs 0 < F <= cout <= 64"),
    ("p4c_out_conv_update_loss_fwd", dict(a=BUF + 8), INVALID, "p4c_out_conv_update_loss_fwd: a and wout must be 16-byte aligned"),
    ("p4c_out_conv_update_loss_fwd", dict(), UNSUPPORTED, NO_PATH_TAIL),
    # ---- p4c_out_conv_update_fwd
    ("p4c_out_conv_update_fwd", dict(border_mask=None), INVALID,
     "p4c_out_conv_update_fwd: null pointer (target, border_mask and interior_mask go together)"),
    ("p4c_out_conv_update_fwd", dict(cout=F - 1), INVALID, "p4c_out_conv_update_loss_fwd: needs 0 < F <= cout <= 64"),
    ("p4c_out_conv_update_fwd", dict(prev=None), INVALID, "p4c_out_conv_update_loss_fwd: prev is null but keep_prev != 0"),
    ("p4c_out_conv_update_fwd", dict(), UNSUPPORTED, NO_PATH_TAIL),
    # ---- p4c_ar_update_loss_bwd_saved
    ("p4c_ar_update_loss_bwd_saved", dict(lgrad=None), INVALID, "p4c_ar_update_loss_bwd_saved: null pointer"),
    ("p4c_ar_update_loss_bwd_saved", dict(dy_dtype=7, g_next2=None), INVALID, "p4c_ar_update_loss_bwd_saved: bad F / y_cs / dtype"),
    ("p4c_ar_update_loss_bwd_saved", dict(g2_dtype=F32), INVALID, "p4c_ar_update_loss_bwd_saved: g_next2 dtype must equal dy dtype"),
    ("p4c_ar_update_loss_bwd_saved", dict(), UNSUPPORTED,
     "p4c_ar_update_loss_bwd_saved: needs the 16-byte path (F % 4 == 0, aligned rows) or the flat path "
     "(F <= 64, N * F % 4 == 0, whole 16-byte slots per row, aligned rows, no NaN masks)"),
    # ---- p4c_ar_update_loss_bwd
    ("p4c_ar_update_loss_bwd", dict(new_state=None), INVALID, "p4c_ar_update_loss_bwd: null pointer"),
    ("p4c_ar_update_loss_bwd", dict(mask_mode=MASK_F32), INVALID, "p4c_ar_update_loss_bwd: only MASK_NONE / MASK_FROM_NAN are fused"),
    ("p4c_ar_update_loss_bwd", dict(g2_dtype=F32), INVALID, "p4c_ar_update_loss_bwd: g_next2 dtype must equal dy dtype"),
    ("p4c_ar_update_loss_bwd", dict(y_cs=300, g2_cs=300), INVALID, "p4c_ar_update_loss_bwd: y_cs too large"),
    ("p4c_ar_update_loss_bwd", dict(dy_dtype=7, g_next2=None), INVALID, "p4c_ar_update_loss_bwd: bad dtype 7"),
    # ---- p4c_ar_update_next_bwd
    ("p4c_ar_update_next_bwd", dict(interior_mask=None), INVALID,
     "p4c_ar_update_next_bwd: null pointer (a forced border needs interior_mask)"),
    ("p4c_ar_update_next_bwd", dict(N=0), INVALID, "p4c_ar_update_next_bwd: null pointer (a forced border needs interior_mask)"),
    ("p4c_ar_update_next_bwd", dict(y_cs=20), INVALID, "p4c_ar_update_loss_bwd: bad F / y_cs"),
    ("p4c_ar_update_next_bwd", dict(g2_dtype=F32), INVALID, "p4c_ar_update_loss_bwd: g_next2 dtype must equal dy dtype"),
]


def test_the_table_covers_every_entry_point():
    from py4cast_amd import _lib

    assert {c[0] for c in CASES} == set(PARAMS)
    for name, params in PARAMS.items():
        assert len(params.split()) == len(_lib.SIGNATURES[name])


@pytest.mark.parametrize("name,override,code,message", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_call_is_refused_before_any_launch(name, override, code, message):
    from py4cast_amd import _lib

    assert set(override) <= set(PARAMS[name].split())
    values = {**BASE, **override}
    handle = _lib.lib()
    rc = getattr(handle, name)(*[values[p] for p in PARAMS[name].split()])
    assert rc == code
    assert handle.p4c_last_error().decode() == message
