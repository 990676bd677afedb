"""UNet (mfai's ``UNet``, py4cast_amd/unet.py) on the host: registry keys, construction from the yaml's settings, state-dict layout
against the float64 restatement (tests/unet_reference.py), the autopad geometry."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from unet_reference import UNetReference  # noqa: E402


def test_registry_has_unet_keys():
    from py4cast_amd import models

    assert "UNet" in models.registry and "UNetMI355X" in models.registry


def test_built_from_yaml_settings():
    from py4cast_amd import models

    kls, settings = models.get_model_kls_and_settings("UNet", {"init_features": 64, "autopad_enabled": True})
    assert settings.init_features == 64 and settings.autopad_enabled is True
    m = kls(69, 60, (64, 64), settings)
    assert m.in_channels == 69 and m.out_channels == 60 and m.features_last and m.is_native_hip
    assert m.supported_num_spatial_dims == (2,) and m.model_type.name == "CONVOLUTIONAL"
    assert "p4c_unet_enc_tail_fwd" in m.timed_entry_points and "p4c_gemm_upconv_fwd" in m.timed_entry_points
    assert not getattr(m, "prefers_hip_graph", False)
    m2, s2 = models.build_model_from_settings("UNet", 69, 60, {"compute_dtype": "bf16", "activation_dtype": "bf16"}, (64, 64))
    assert s2.compute_dtype == "bf16" and m2.native


def test_positional_and_keyword_construction():
    from py4cast_amd.unet import UNetMI355X, UNetSettings

    s = UNetSettings(init_features=16)
    a = UNetMI355X(5, 3, (32, 32), s)
    b = UNetMI355X(in_channels=5, out_channels=3, input_shape=(32, 32), settings=s)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(sa[k].shape == sb[k].shape for k in sa)


@pytest.mark.parametrize("cin,cout,f", [(69, 60, 64), (2, 1, 64)])
def test_state_dict_matches_restatement(cin, cout, f):
    from py4cast_amd.unet import UNetMI355X, UNetSettings

    m = UNetMI355X(cin, cout, (64, 64), UNetSettings(init_features=f))
    ref = UNetReference(cin, cout, f)
    sm, sr = m.state_dict(), ref.state_dict()
    assert list(sm) == list(sr)
    for k in sr:
        assert sm[k].shape == sr[k].shape, k
    for k in ("encoder1.enc1conv1.weight", "encoder1.enc1norm1.num_batches_tracked", "bottleneck.bottleneckconv1.weight",
              "upconv4.weight", "upconv4.bias", "decoder4.dec4conv1.weight", "conv.weight", "conv.bias"):
        assert k in sm
    assert m.load_state_dict(sr) is not None


def test_padding_for_matches_halfunet():
    from py4cast_amd.halfunet import HalfUNetMI355X
    from py4cast_amd.unet import UNetMI355X, UNetSettings

    m = UNetMI355X(2, 1, (70, 64), UNetSettings())
    for hw in ((70, 64), (56, 72), (64, 64), (17, 31)):
        assert m.padding_for(*hw) == HalfUNetMI355X.padding_for(None, *hw)
    assert m.padding_for(70, 64) == (5, 5, 0, 0)


def test_unserved_dtype_settings_are_rejected():
    from py4cast_amd.unet import UNetMI355X, UNetSettings

    with pytest.raises(ValueError):
        UNetMI355X(2, 1, (64, 64), UNetSettings(init_features=12, compute_dtype="bf16"))
    with pytest.raises(ValueError):
        UNetMI355X(2, 1, (64, 64), UNetSettings(compute_dtype="bf16", activation_dtype="f32"))
    with pytest.raises(ValueError):
        UNetMI355X(2, 1, (64, 64), UNetSettings(compute_dtype="f32", activation_dtype="bf16"))
    assert UNetMI355X(2, 1, (64, 64), UNetSettings(init_features=12)).act_dtype.is_floating_point   # fp32: any width
