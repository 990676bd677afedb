"""DeepLabV3+ (smp's DeepLabV3Plus as mfai builds it, py4cast_amd/deeplabv3plus.py) on the host: registry keys, construction from the yaml's
settings with no checkpoint anywhere (a warning, never a download), the state-dict layout written out by hand, the output-stride-16
encoder geometry, unserved settings, the grid check, encoder weights from a local torchvision-keyed checkpoint, and the fp32 flavour
(library operations, on the CPU) against the float64 restatement (tests/deeplabv3plus_reference.py)."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from deeplabv3plus_reference import DeepLabV3PlusReference  # noqa: E402

# config/CLI/model/deeplabv3plus.yaml: settings_init_args
YAML = {"encoder_name": "resnet18", "encoder_depth": 5, "encoder_weights": True, "decoder_channels": 256, "activation": None, "upsampling": 8,
        "aux_params": None}


@pytest.fixture
def empty_hub(tmp_path, monkeypatch):
    """torch.hub's directory pointed at an empty tmp dir: no checkpoint to find, nothing to fetch"""
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    return tmp_path / "hub"


def test_registry_has_deeplabv3plus_keys():
    from py4cast_amd import models

    assert "DeepLabV3Plus" in models.registry and "DeepLabV3PlusMI355X" in models.registry
    # with this model every key of the reference's registry (its tests/test_models.py) is served
    assert {"HalfUNet", "UNet", "CustomUNet", "Segformer", "SwinUNetR", "UNetRPP", "DeepLabV3", "DeepLabV3Plus", "HiLAM", "GraphLAM",
            "HiLAMParallel", "Identity"} <= set(models.registry)


def test_built_from_yaml_settings_warns_and_fetches_nothing(empty_hub, monkeypatch):
    from py4cast_amd import deeplabv3, models

    def no_fetch(*a, **k):
        raise AssertionError("a download was attempted")

    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_fetch)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_fetch)
    monkeypatch.setattr(deeplabv3, "_WARNED", set())
    with pytest.warns(UserWarning, match="DeepLabV3PlusMI355X: no resnet18 checkpoint found .* random initialisation"):
        m, s = models.build_model_from_settings("DeepLabV3Plus", 69, 60, dict(YAML), (64, 64))
    assert s.encoder_name == "resnet18" and s.decoder_channels == 256 and s.upsampling == 8 and s.compute_dtype == "f32" and s.aspp_dropout == 0.5
    assert m.in_channels == 69 and m.out_channels == 60 and m.features_last and m.is_native_hip and not m.native
    assert m.supported_num_spatial_dims == (2,) and m.model_type.name == "CONVOLUTIONAL"
    for name in ("p4c_dlp_dw3x3_fwd", "p4c_dlp_dw3x3_dgrad", "p4c_dlp_dw3x3_wgrad", "p4c_dlp_up_cat_fwd", "p4c_dlp_up_cat_bwd"):
        assert name in m.timed_entry_points
    assert m.last_dropout_mask is None and isinstance(m.prefers_hip_graph, bool)
    assert m.encoder.conv1.weight.shape == (64, 69, 7, 7) and m.rollout_input_format is None
    # the head up-samples x4 whatever the yaml's `upsampling` (8) says: the output is on the input's grid
    assert m.segmentation_head[1].scale_factor == 4 and m.decoder.up.scale_factor == 4
    m.eval()
    with torch.no_grad():
        assert m(torch.zeros(1, 32, 48, 69)).shape == (1, 32, 48, 60)
    kls, s2 = models.get_model_kls_and_settings("DeepLabV3Plus", {"compute_dtype": "bf16", "activation_dtype": "bf16", "encoder_weights": False})
    nat = kls(69, 60, (64, 64), s2)
    assert nat.native and nat.rollout_input_format == (torch.bfloat16, 72) and s2.upsampling == 4


def _bn_keys(prefix, c):
    return [(f"{prefix}.weight", (c,)), (f"{prefix}.bias", (c,)), (f"{prefix}.running_mean", (c,)), (f"{prefix}.running_var", (c,)),
            (f"{prefix}.num_batches_tracked", ())]


def _expected_resnet18_keys(cin, cout, dc=256):
    """the state dict of the resnet18 model, key by key in registration order, written from the issue's layout (not from the code)"""
    keys = [("encoder.conv1.weight", (64, cin, 7, 7))] + _bn_keys("encoder.bn1", 64)
    ci = 64
    for layer, co in ((1, 64), (2, 128), (3, 256), (4, 512)):
        for j in range(2):
            p = f"encoder.layer{layer}.{j}"
            keys += [(f"{p}.conv1.weight", (co, ci, 3, 3))] + _bn_keys(f"{p}.bn1", co)
            keys += [(f"{p}.conv2.weight", (co, co, 3, 3))] + _bn_keys(f"{p}.bn2", co)
            if j == 0 and ci != co:
                keys += [(f"{p}.downsample.0.weight", (co, ci, 1, 1))] + _bn_keys(f"{p}.downsample.1", co)
            ci = co
    a = "decoder.aspp.0"
    keys += [(f"{a}.convs.0.0.weight", (dc, 512, 1, 1))] + _bn_keys(f"{a}.convs.0.1", dc)
    for k in (1, 2, 3):
        keys += [(f"{a}.convs.{k}.0.0.weight", (512, 1, 3, 3)), (f"{a}.convs.{k}.0.1.weight", (dc, 512, 1, 1))] + _bn_keys(f"{a}.convs.{k}.1", dc)
    keys += [(f"{a}.convs.4.1.weight", (dc, 512, 1, 1))] + _bn_keys(f"{a}.convs.4.2", dc)
    keys += [(f"{a}.project.0.weight", (dc, 5 * dc, 1, 1))] + _bn_keys(f"{a}.project.1", dc)
    keys += [("decoder.aspp.1.0.weight", (dc, 1, 3, 3)), ("decoder.aspp.1.1.weight", (dc, dc, 1, 1))] + _bn_keys("decoder.aspp.2", dc)
    keys += [("decoder.block1.0.weight", (48, 64, 1, 1))] + _bn_keys("decoder.block1.1", 48)
    keys += [("decoder.block2.0.0.weight", (dc + 48, 1, 3, 3)), ("decoder.block2.0.1.weight", (dc, dc + 48, 1, 1))] + _bn_keys("decoder.block2.1", dc)
    keys += [("segmentation_head.0.weight", (cout, dc, 1, 1)), ("segmentation_head.0.bias", (cout,))]
    return keys


@pytest.mark.parametrize("cin,cout", [(69, 60), (11, 4)])
def test_state_dict_layout_resnet18(cin, cout):
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    m = DeepLabV3PlusMI355X(cin, cout, (64, 64), DeepLabV3PlusSettings(encoder_weights=False))
    sm = m.state_dict()
    want = _expected_resnet18_keys(cin, cout)
    assert list(sm) == [k for k, _ in want]
    for k, shape in want:
        assert tuple(sm[k].shape) == shape, (k, tuple(sm[k].shape), shape)
    assert sm["encoder.layer4.0.conv1.weight"].shape == (512, 256, 3, 3)
    assert sm["decoder.aspp.0.convs.1.0.0.weight"].shape == (512, 1, 3, 3) and sm["decoder.aspp.0.convs.1.0.1.weight"].shape == (256, 512, 1, 1)
    assert sm["decoder.aspp.0.project.0.weight"].shape == (256, 1280, 1, 1) and sm["decoder.aspp.1.0.weight"].shape == (256, 1, 3, 3)
    assert sm["decoder.block1.0.weight"].shape == (48, 64, 1, 1) and sm["decoder.block2.0.0.weight"].shape == (304, 1, 3, 3)
    assert sm["decoder.block2.0.1.weight"].shape == (256, 304, 1, 1) and sm["segmentation_head.0.weight"].shape == (cout, 256, 1, 1)
    assert not any(k.startswith("encoder.fc") for k in sm)


@pytest.mark.parametrize("name", ["resnet18", "resnet34"])
def test_state_dict_matches_restatement_and_encoder_geometry(name):
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    m = DeepLabV3PlusMI355X(11, 4, (64, 64), DeepLabV3PlusSettings(encoder_name=name, encoder_weights=False, decoder_channels=32))
    ref = DeepLabV3PlusReference(11, 4, name, decoder_channels=32)
    sm, sr = m.state_dict(), ref.state_dict()
    assert list(sm) == list(sr)
    for k in sr:
        assert sm[k].shape == sr[k].shape, k
    m.load_state_dict(sr)
    enc = m.encoder
    # output stride 16: layer2 and layer3 keep their stride 2 (first block), layer4 runs at stride 1, dilation 2, padding 2
    for layer in (enc.layer2, enc.layer3):
        assert layer[0].conv1.stride == (2, 2) and layer[0].downsample[0].stride == (2, 2) and layer[1].conv1.stride == (1, 1)
        assert all(c.dilation == (1, 1) for c in layer.modules() if isinstance(c, torch.nn.Conv2d))
    for c in (c for c in enc.layer4.modules() if isinstance(c, torch.nn.Conv2d)):
        assert c.stride == (1, 1), c
        if c.kernel_size == (3, 3):
            assert c.dilation == (2, 2) and c.padding == (2, 2), c
    assert enc.layer4[0].downsample is not None and enc.layer1[0].downsample is None
    # the separable ASPP: depthwise at padding = dilation = rate, no bias anywhere in the decoder
    for k, r in zip((1, 2, 3), (12, 24, 36)):
        dw, pw = m.decoder.aspp[0].convs[k][0][0], m.decoder.aspp[0].convs[k][0][1]
        assert dw.groups == 512 and dw.dilation == (r, r) and dw.padding == (r, r) and dw.bias is None and pw.bias is None
    assert all(c.bias is None for c in m.decoder.modules() if isinstance(c, torch.nn.Conv2d))
    assert m.decoder.block2[0][0].groups == 32 + 48 and m.decoder.block2[0][0].padding == (1, 1)


@pytest.mark.parametrize("field,value", [("upsampling", 2), ("upsampling", 16), ("activation", "sigmoid"), ("aux_params", {"classes": 3}),
                                         ("encoder_depth", 4), ("decoder_channels", 20), ("decoder_channels", 0), ("encoder_name", "resnet50"),
                                         ("encoder_name", "mobilenet_v2"), ("aspp_dropout", 1.0), ("compute_dtype", "f16")])
def test_unserved_settings_raise(field, value):
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    with pytest.raises(ValueError, match="DeepLabV3PlusMI355X"):
        DeepLabV3PlusMI355X(3, 1, (64, 64), DeepLabV3PlusSettings(encoder_weights=False, **{field: value}))


@pytest.mark.parametrize("upsampling", [4, 8])
def test_served_upsampling_values(upsampling):
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    m = DeepLabV3PlusMI355X(3, 1, (64, 64), DeepLabV3PlusSettings(encoder_weights=False, upsampling=upsampling))
    assert m.segmentation_head[1].scale_factor == 4


def test_grid_must_be_a_multiple_of_16():
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    m = DeepLabV3PlusMI355X(3, 1, None, DeepLabV3PlusSettings(encoder_weights=False))
    with pytest.raises(RuntimeError, match=r"Wrong input shape height=72, width=64\. Expected image height and width divisible by 16\. "
                                           r"Consider pad your images to shape \(80, 64\)\."):
        m(torch.zeros(2, 72, 64, 3))
    m.check_grid(64, 96)


@pytest.mark.parametrize("cin", [3, 5, 69, 1])
def test_encoder_weights_from_path(tmp_path, empty_hub, cin):
    from py4cast_amd.deeplabv3 import ResNetEncoder
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    g = torch.Generator().manual_seed(0)
    enc = ResNetEncoder(3, (2, 2, 2, 2))
    sd = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v) for k, v in enc.state_dict().items()}
    sd["fc.weight"] = torch.randn(1000, 512, generator=g)
    sd["fc.bias"] = torch.randn(1000, generator=g)
    path = tmp_path / "resnet18-local.pth"
    torch.save(sd, path)
    with warnings.catch_warnings():
        warnings.simplefilter("error")        # a found checkpoint loads without any warning
        m = DeepLabV3PlusMI355X(cin, 2, (64, 64), DeepLabV3PlusSettings(encoder_weights_path=str(path)))
    got = m.encoder.state_dict()
    for k, v in sd.items():
        if k.startswith("fc.") or k == "conv1.weight":
            continue
        assert torch.equal(got[k], v), k
    w = sd["conv1.weight"]
    if cin == 3:
        want = w
    elif cin == 1:
        want = w.sum(1, keepdim=True)
    else:
        want = torch.stack([w[:, i % 3] for i in range(cin)], dim=1) * (3 / cin)
    assert torch.allclose(got["conv1.weight"], want, rtol=0, atol=1e-6)


def test_initialisation():
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    torch.manual_seed(0)
    m = DeepLabV3PlusMI355X(8, 60, (64, 64), DeepLabV3PlusSettings(encoder_weights=False))
    assert torch.equal(m.segmentation_head[0].bias.detach(), torch.zeros(60))
    assert all(torch.equal(b.weight.detach(), torch.ones_like(b.weight)) and torch.equal(b.bias.detach(), torch.zeros_like(b.bias))
               for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))
    # kaiming-normal fan_out: std sqrt(2 / (64 * 49)) for conv1; kaiming-uniform fan_in: bound sqrt(6 / 9) for a depthwise 3x3 (fan_in 9),
    # sqrt(6 / 304) for block2's pointwise; xavier-uniform: bound sqrt(6 / (256 + 60)) for the head
    assert abs(float(m.encoder.conv1.weight.detach().std()) - (2 / (64 * 49)) ** 0.5) < 0.1 * (2 / (64 * 49)) ** 0.5
    dw = m.decoder.aspp[0].convs[2][0][0].weight.detach()
    assert (6 / 9) ** 0.5 * 0.9 <= float(dw.abs().max()) <= (6 / 9) ** 0.5
    assert float(m.decoder.block2[0][1].weight.detach().abs().max()) <= (6 / 304) ** 0.5
    assert float(m.segmentation_head[0].weight.detach().abs().max()) <= (6 / 316) ** 0.5


def test_training_needs_two_samples_for_the_pooling_branch():
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    m = DeepLabV3PlusMI355X(3, 1, None, DeepLabV3PlusSettings(encoder_weights=False, decoder_channels=8)).train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(torch.zeros(1, 32, 32, 3))


def test_native_nodes_have_no_cpu_path():
    from py4cast_amd._lib import P4CError
    from py4cast_amd.deeplabv3plus import depthwise3x3_dilated, up_cat

    x = torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16)
    with pytest.raises(P4CError):
        depthwise3x3_dilated(x, [torch.zeros(8, 1, 3, 3)], (1,))
    with pytest.raises(P4CError):
        up_cat(x, torch.zeros(1, 16, 16, 8, dtype=torch.bfloat16), 4)


@pytest.mark.parametrize("name", ["resnet18", "resnet34"])
def test_fp32_flavour_on_cpu_against_float64(name):
    """the fp32 flavour (the model's own module tree on library operations) against the float64 restatement at 2 x 128 x 96, 5 -> 3
    channels, dc = 32: train mode with batch statistics, then eval; 5e-4 relative"""
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    torch.manual_seed(1)
    cin, cout, H, W = 5, 3, 128, 96
    m = DeepLabV3PlusMI355X(cin, cout, (H, W), DeepLabV3PlusSettings(encoder_name=name, encoder_weights=False, decoder_channels=32,
                                                                     aspp_dropout=0.0)).train()
    ref = DeepLabV3PlusReference(cin, cout, name, decoder_channels=32).double().train()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in m.state_dict().items()})
    x = torch.randn(2, H, W, cin)
    got, want = m(x), ref(x.double())
    assert got.shape == want.shape == (2, H, W, cout) and got.dtype == torch.float32

    def rel(a, b):
        return float((a.detach().double() - b.detach()).norm() / b.detach().norm())

    print(f"\n{name} train out {rel(got, want):.3e}")
    assert rel(got, want) <= 5e-4, rel(got, want)
    assert rel(m.decoder.block2[1].running_mean, ref.decoder.block2[1].running_mean) <= 5e-4
    m.eval()
    ref.eval()
    with torch.no_grad():
        ge, we = m(x), ref(x.double())
    print(f"{name} eval out {rel(ge, we):.3e}")
    assert rel(ge, we) <= 5e-4
