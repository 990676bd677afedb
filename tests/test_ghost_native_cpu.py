"""HalfUNet with Ghost blocks: which settings take the native bf16 route (``ghost_native``), and what stays as it was for every Ghost
model -- ``module_path``, no native rollout, mfai's parameter and buffer names.  No GPU."""
import pytest

BF16 = dict(compute_dtype="bf16", activation_dtype="bf16")


def build(**kw):
    from py4cast_amd.halfunet import HalfUNetMI355X, HalfUNetSettings

    return HalfUNetMI355X(21, 12, (48, 64), HalfUNetSettings(**kw))


def test_ghost_native_for_the_yaml_settings_in_bf16():
    m = build(use_ghost=True, **BF16)
    assert m.ghost_native is True
    assert m.module_path is True and m.native_rollout is None
    assert build(use_ghost=True, compute_dtype="bf16").ghost_native is True      # activation_dtype None = compute_dtype
    with pytest.raises(AttributeError):
        m.ghost_native = False
    for name in ("p4c_ghost_tail_fwd", "p4c_ghost_tail_bwd", "p4c_halfunet_merge_fwd", "p4c_halfunet_merge_bwd", "p4c_gemm_nt", "p4c_gemm_tn",
                 "p4c_unet_enc_tail_fwd", "p4c_unet_enc_tail_bwd", "p4c_inorm_apply"):
        assert name in m.timed_entry_points, name


@pytest.mark.parametrize("kw", [
    dict(use_ghost=True),                                             # fp32
    dict(use_ghost=True, compute_dtype="bf16", activation_dtype="f32"),
    dict(use_ghost=True, bias=True, **BF16),
    dict(use_ghost=True, num_filters=48, **BF16),
    dict(use_ghost=True, dilation=2, **BF16),
    dict(use_ghost=True, norm="group", **BF16),
    dict(use_ghost=True, last_activation="Sigmoid", **BF16),
    dict(use_ghost=False, **BF16),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_ghost_native_is_off_elsewhere(kw):
    m = build(**kw)
    assert m.ghost_native is False
    if kw["use_ghost"]:
        assert m.module_path is True and m.native_rollout is None
    else:
        assert m.module_path is False and callable(m.native_rollout)


def test_ghost_state_dict_keeps_mfai_names():
    from oracle.halfunet import HalfUNetRef

    m = build(use_ghost=True, **BF16)
    ref = HalfUNetRef(21, 12, use_ghost=True)
    assert list(m.state_dict()) == list(build(use_ghost=True).state_dict())
    assert set(m.state_dict()) == set(ref.state_dict())
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert m.grad_input_channels == 21
    assert m.padding_for(40, 72) == (4, 4, 4, 4)
