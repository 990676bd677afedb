"""DeepLabV3 (smp's network as mfai builds it, py4cast_amd/deeplabv3.py) on the host: registry keys, construction from the yaml's settings,
the state-dict layout against the float64 restatement (tests/deeplabv3_reference.py), unserved settings, encoder weights from a local
torchvision-keyed checkpoint (never a download), and the restatement against the module tree's library forward."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from deeplabv3_reference import DeepLabV3Reference  # noqa: E402

YAML = {"encoder_name": "resnet18", "encoder_depth": 5, "encoder_weights": True, "decoder_channels": 256, "activation": None,
        "upsampling": 8, "aux_params": None}


@pytest.fixture
def empty_hub(tmp_path, monkeypatch):
    """torch.hub's directory pointed at an empty tmp dir: no checkpoint to find, nothing to fetch"""
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    return tmp_path / "hub"


def test_registry_has_deeplabv3_keys():
    from py4cast_amd import models

    assert "DeepLabV3" in models.registry and "DeepLabV3MI355X" in models.registry


def test_built_from_yaml_settings(empty_hub):
    from py4cast_amd import models

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m, s = models.build_model_from_settings("DeepLabV3", 69, 60, dict(YAML), (64, 64))
    assert s.encoder_name == "resnet18" and s.decoder_channels == 256 and s.upsampling == 8
    assert m.in_channels == 69 and m.out_channels == 60 and m.features_last and m.is_native_hip
    assert m.supported_num_spatial_dims == (2,) and m.model_type.name == "CONVOLUTIONAL"
    assert "p4c_deeplab_stem_fwd" in m.timed_entry_points and "p4c_upsample_bilinear_ac_fwd" in m.timed_entry_points
    assert m.encoder.conv1.weight.shape == (64, 69, 7, 7)
    kls, s2 = models.get_model_kls_and_settings("DeepLabV3", {"compute_dtype": "bf16", "activation_dtype": "bf16"})
    assert s2.encoder_weights is True and s2.aspp_dropout == 0.5
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert kls(69, 60, (64, 64), s2).native


@pytest.mark.parametrize("name", ["resnet18", "resnet34"])
@pytest.mark.parametrize("cin,cout,dc", [(69, 60, 256), (3, 1, 64)])
def test_state_dict_matches_restatement(name, cin, cout, dc):
    from py4cast_amd.deeplabv3 import DeepLabV3MI355X, DeepLabV3Settings

    m = DeepLabV3MI355X(cin, cout, (64, 64), DeepLabV3Settings(encoder_name=name, decoder_channels=dc, encoder_weights=False))
    ref = DeepLabV3Reference(cin, cout, name, dc)
    sm, sr = m.state_dict(), ref.state_dict()
    assert list(sm) == list(sr)
    for k in sr:
        assert sm[k].shape == sr[k].shape, k
    for k in ("encoder.conv1.weight", "encoder.bn1.num_batches_tracked", "encoder.layer2.0.downsample.0.weight",
              "encoder.layer4.1.conv2.weight", "decoder.0.convs.0.0.weight", "decoder.0.convs.3.0.weight", "decoder.0.convs.4.1.weight",
              "decoder.0.convs.4.2.running_var", "decoder.0.project.0.weight", "decoder.1.weight", "decoder.2.bias",
              "segmentation_head.0.weight", "segmentation_head.0.bias"):
        assert k in sm, k
    assert not any(k.startswith("encoder.fc") for k in sm)
    assert m.load_state_dict(sr) is not None
    # output stride 8: layer3 / layer4 dilated, stride 1
    assert m.encoder.layer3[0].conv1.dilation == (2, 2) and m.encoder.layer3[0].conv1.stride == (1, 1)
    assert m.encoder.layer4[0].conv2.padding == (4, 4) and m.encoder.layer4[0].downsample[0].stride == (1, 1)
    assert m.encoder.layer2[0].conv1.stride == (2, 2)


@pytest.mark.parametrize("field,value", [("encoder_name", "resnet50"), ("encoder_name", "mobilenet_v2"), ("encoder_depth", 4),
                                         ("decoder_channels", 100), ("activation", "sigmoid"), ("upsampling", 4), ("upsampling", 1),
                                         ("aux_params", {"classes": 3}), ("aspp_dropout", 1.0), ("compute_dtype", "f16")])
def test_unserved_settings_raise(field, value):
    from py4cast_amd.deeplabv3 import DeepLabV3MI355X, DeepLabV3Settings

    with pytest.raises(ValueError):
        DeepLabV3MI355X(3, 1, (64, 64), DeepLabV3Settings(encoder_weights=False, **{field: value}))


def test_unserved_dtype_combinations_raise():
    from py4cast_amd.deeplabv3 import DeepLabV3MI355X, DeepLabV3Settings

    for cd, ad in (("bf16", "f32"), ("f32", "bf16")):
        with pytest.raises(ValueError):
            DeepLabV3MI355X(3, 1, (64, 64), DeepLabV3Settings(encoder_weights=False, compute_dtype=cd, activation_dtype=ad))


def _torchvision_checkpoint(path, seed=0):
    """a synthetic resnet18 state dict with torchvision's key names (fc included)"""
    from py4cast_amd.deeplabv3 import ResNetEncoder

    g = torch.Generator().manual_seed(seed)
    enc = ResNetEncoder(3, (2, 2, 2, 2))
    sd = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v) for k, v in enc.state_dict().items()}
    sd["fc.weight"] = torch.randn(1000, 512, generator=g)
    sd["fc.bias"] = torch.randn(1000, generator=g)
    torch.save(sd, path)
    return sd


@pytest.mark.parametrize("cin", [3, 5, 69, 1])
def test_encoder_weights_from_path(tmp_path, empty_hub, cin):
    from py4cast_amd.deeplabv3 import DeepLabV3MI355X, DeepLabV3Settings

    path = tmp_path / "resnet18-local.pth"
    sd = _torchvision_checkpoint(path)
    with warnings.catch_warnings():
        warnings.simplefilter("error")        # a found checkpoint loads without any warning
        m = DeepLabV3MI355X(cin, 2, (64, 64), DeepLabV3Settings(encoder_weights_path=str(path)))
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


def test_encoder_weights_from_hub_cache(empty_hub):
    from py4cast_amd.deeplabv3 import DeepLabV3MI355X, DeepLabV3Settings

    os.makedirs(empty_hub / "checkpoints")
    sd = _torchvision_checkpoint(empty_hub / "checkpoints" / "resnet18-f37072fd.pth", seed=3)
    m = DeepLabV3MI355X(3, 2, (64, 64), DeepLabV3Settings())
    assert torch.equal(m.encoder.layer3[1].conv2.weight.detach(), sd["layer3.1.conv2.weight"])


def test_missing_checkpoint_warns_and_fetches_nothing(empty_hub, monkeypatch):
    from py4cast_amd import deeplabv3
    from py4cast_amd.deeplabv3 import DeepLabV3MI355X, DeepLabV3Settings

    def no_fetch(*a, **k):
        raise AssertionError("a download was attempted")

    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_fetch)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_fetch)
    monkeypatch.setattr(deeplabv3, "_WARNED", set())
    with pytest.warns(UserWarning, match="random initialisation"):
        a = DeepLabV3MI355X(3, 2, (64, 64), DeepLabV3Settings(encoder_name="resnet34"))
    with warnings.catch_warnings():
        warnings.simplefilter("error")        # once per encoder name
        DeepLabV3MI355X(3, 2, (64, 64), DeepLabV3Settings(encoder_name="resnet34"))
    assert a.encoder.conv1.weight.shape == (64, 3, 7, 7)


def test_initialisation_follows_smp():
    from py4cast_amd.deeplabv3 import DeepLabV3MI355X, DeepLabV3Settings

    torch.manual_seed(0)
    m = DeepLabV3MI355X(8, 60, (64, 64), DeepLabV3Settings(encoder_weights=False))
    assert torch.equal(m.segmentation_head[0].bias.detach(), torch.zeros(60))
    assert all(torch.equal(b.weight.detach(), torch.ones_like(b.weight)) and torch.equal(b.bias.detach(), torch.zeros_like(b.bias))
               for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))
    # kaiming-normal fan_out: std sqrt(2 / (64 * 49)) for conv1; kaiming-uniform fan_in: bound sqrt(6 / (512 * 9)) for convs.1
    assert abs(float(m.encoder.conv1.weight.detach().std()) - (2 / (64 * 49)) ** 0.5) < 0.1 * (2 / (64 * 49)) ** 0.5
    assert float(m.decoder[0].convs[1][0].weight.detach().abs().max()) <= (6 / (512 * 9)) ** 0.5


@pytest.mark.parametrize("name,H,W", [("resnet18", 64, 64), ("resnet34", 64, 96)])
def test_restatement_matches_module_tree(name, H, W):
    """the restatement (torch.nn.functional) against the model's own module tree (nn.Conv2d / MaxPool2d / UpsamplingBilinear2d / cat):
    two independent statements of the same network, float64, train mode with batch statistics, dropout off"""
    from py4cast_amd.deeplabv3 import DeepLabV3MI355X, DeepLabV3Settings

    torch.manual_seed(1)
    m = DeepLabV3MI355X(5, 3, (H, W), DeepLabV3Settings(encoder_name=name, decoder_channels=32, encoder_weights=False,
                                                         aspp_dropout=0.0)).double()
    ref = DeepLabV3Reference(5, 3, name, 32).double()
    ref.load_state_dict(m.state_dict())
    x = torch.randn(2, H, W, 5, dtype=torch.float64)
    want = ref(x)
    got = m.segmentation_head(m.decoder(m.encoder(x.permute(0, 3, 1, 2)))).permute(0, 2, 3, 1)
    assert got.shape == (2, H, W, 3)
    assert torch.allclose(got, want, rtol=1e-10, atol=1e-10)
    # running statistics moved the same way
    assert torch.allclose(m.decoder[0].convs[4][2].running_mean, ref.decoder[0].convs[4][2].running_mean, atol=1e-12)
    m.eval()
    ref.eval()
    assert torch.allclose(m.segmentation_head(m.decoder(m.encoder(x.permute(0, 3, 1, 2)))).permute(0, 2, 3, 1), ref(x), rtol=1e-10,
                          atol=1e-10)
