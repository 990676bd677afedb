"""Segformer (mfai's ``Segformer``, py4cast_amd/segformer.py) on the host: registry keys, construction from the yaml's settings,
state-dict layout against the float64 restatement (tests/segformer_reference.py), the grid rule, and the fp32 route (library
operations) against the restatement, forward and gradients."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from segformer_reference import SegformerReference, ref_forward_nhwc, reference_from  # noqa: E402

YAML_SETTINGS = {"num_layers": 2, "decoder_dim": 256, "num_downsampling_chans": 32}


def test_registry_has_segformer_keys():
    from py4cast_amd import models

    assert "Segformer" in models.registry and "SegformerMI355X" in models.registry


def test_built_from_yaml_settings():
    from py4cast_amd import models

    m, s = models.build_model_from_settings("Segformer", 69, 60, YAML_SETTINGS, (512, 512))
    assert s.num_layers == 2 and s.decoder_dim == 256 and tuple(s.dims) == (32, 64, 160, 256) and tuple(s.heads) == (1, 2, 5, 8)
    assert m.in_channels == 69 and m.out_channels == 60 and m.features_last and m.is_native_hip and not m.onnx_supported
    assert m.model_type.name == "VISION_TRANSFORMER" and m.rollout_input_format is None
    m2, s2 = models.build_model_from_settings("Segformer", 69, 60, dict(YAML_SETTINGS, compute_dtype="bf16"), (512, 640))
    assert m2.native and m2.rollout_input_format == (torch.bfloat16, 72)
    assert "p4c_seg_sra_fwd" in m2.timed_entry_points


@pytest.mark.parametrize("cin,cout", [(69, 60), (2, 1)])
def test_state_dict_matches_restatement(cin, cout):
    from py4cast_amd.segformer import SegformerMI355X, SegformerSettings

    m = SegformerMI355X(cin, cout, (64, 64), SegformerSettings())
    ref = SegformerReference(cin, cout)
    sm, sr = m.state_dict(), ref.state_dict()
    assert list(sm) == list(sr)
    for k in sr:
        assert sm[k].shape == sr[k].shape, k
    for k in ("downsampler.weight", "mit.stages.0.1.weight", "mit.stages.3.2.1.0.norm.g", "mit.stages.1.2.0.0.fn.to_kv.weight",
              "mit.stages.2.2.1.1.fn.net.1.net.0.weight", "mit.stages.2.2.1.1.fn.net.1.net.1.bias", "mit.stages.0.2.0.1.fn.net.3.weight",
              "to_fused.3.0.weight", "to_segmentation.1.bias"):
        assert k in sm, k
    assert m.load_state_dict(sr) is not None
    assert ref.load_state_dict(sm) is not None


@pytest.mark.parametrize("grid", [(96, 64), (64, 100), (32, 32)])
def test_grid_not_multiple_of_64_rejected(grid):
    from py4cast_amd.segformer import SegformerMI355X, SegformerSettings

    for dt in ("f32", "bf16"):
        with pytest.raises(ValueError):
            SegformerMI355X(4, 3, grid, SegformerSettings(compute_dtype=dt))


def test_unserved_native_settings_rejected():
    from py4cast_amd.segformer import SegformerMI355X, SegformerSettings

    with pytest.raises(ValueError):        # head_dim 64
        SegformerMI355X(4, 3, (64, 64), SegformerSettings(heads=(1, 1, 5, 8), compute_dtype="bf16"))
    with pytest.raises(ValueError):        # 1024 keys per stage
        SegformerMI355X(4, 3, (2048, 2048), SegformerSettings(compute_dtype="bf16"))
    with pytest.raises(ValueError):        # a channel count off the GEMM's 8-channel granularity
        SegformerMI355X(4, 3, (64, 64), SegformerSettings(num_downsampling_chans=36, compute_dtype="bf16"))
    # the fp32 route serves any head_dim and key count
    SegformerMI355X(4, 3, (64, 64), SegformerSettings(heads=(1, 1, 5, 8)))
    SegformerMI355X(4, 3, (2048, 2048), SegformerSettings())


@pytest.mark.parametrize("grid", [(64, 64), (128, 192)])
def test_f32_route_matches_restatement(grid):
    from py4cast_amd.segformer import SegformerMI355X, SegformerSettings

    torch.manual_seed(0)
    H, W = grid
    m = SegformerMI355X(5, 3, grid, SegformerSettings())
    with torch.no_grad():          # non-trivial norms
        for n, p in m.named_parameters():
            if n.endswith("norm.g") or n.endswith("norm.b"):
                p.add_(0.1 * torch.randn_like(p))
    ref = reference_from(m)
    x = torch.randn(2, H, W, 5)
    x64 = x.double().requires_grad_(True)
    x32 = x.clone().requires_grad_(True)
    y = m(x32)
    yr = ref_forward_nhwc(ref, x64)
    assert y.shape == (2, H, W, 3)
    rel = ((y.double() - yr).norm() / yr.norm()).item()
    assert rel < 1e-4, rel
    g = torch.randn_like(yr)
    (y.double() * g).sum().backward()
    (yr * g).sum().backward()
    rel = ((x32.grad.double() - x64.grad).norm() / x64.grad.norm()).item()
    assert rel < 1e-4, rel
    pr = dict(ref.named_parameters())
    for n, p in m.named_parameters():
        gr = pr[n].grad
        rel = ((p.grad.double() - gr).norm() / gr.norm().clamp_min(1e-30)).item()
        assert rel < 1e-4, (n, rel)
