"""The device-free half of tests/test_segformer_settings_bf16_gpu.py: the four configurations of tests/segformer_settings_cases.py in the f32
flavour on the CPU against the float64 restatement built WITH THE SAME SETTINGS (1e-4), the condition of the device's block checks (every
block's own part at least 0.05 of its input, in float64 alone), the float64 references of the nodes outside the blocks
(tests/segformer_nodes.py) against plain torch modules (1e-12), the recorder's undo, and the constructor's refusal of more than 256 keys."""
import os
import sys

import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import segformer_nodes as N  # noqa: E402
import segformer_reference as R  # noqa: E402
import segformer_settings_cases as C  # noqa: E402


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


_RUNS = {}


def _run(name):
    """the f32 model and its float64 restatement, one forward / backward each on the table's grid; the restatement's blocks hooked"""
    if name not in _RUNS:
        C.assert_case_shapes(name)
        m = C.make_model(name, "f32")
        C.assert_case_shapes(name, m)
        ref = R.reference_from(m)
        own = []
        # (a PreNorm returns the block's own part fn(norm(x)); the residual is added outside it)
        hooks = [mod.register_forward_hook(lambda mod, args, out: own.append(float(out.detach().norm() / args[0].detach().norm())))
                 for mod in ref.modules() if isinstance(mod, R.PreNorm)]
        x, dy = C.make_inputs(name)
        xg = x.clone().requires_grad_(True)
        y = m(xg)
        y.backward(dy)
        xd = x.double().requires_grad_(True)
        yr = R.ref_forward_nhwc(ref, xd)
        yr.backward(dy.double())
        for h in hooks:
            h.remove()
        _RUNS[name] = dict(m=m, ref=ref, y=y.detach(), yr=yr.detach(), dx=xg.grad, dxr=xd.grad, own=own)
    return _RUNS[name]


@pytest.mark.parametrize("name", C.NAMES)
def test_f32_flavour_against_float64(name):
    r = _run(name)
    c = C.CASES[name]
    assert r["y"].shape == r["yr"].shape == (c["B"], *c["grid"], c["cout"])
    assert rel(r["y"], r["yr"]) <= 1e-4 and rel(r["dx"], r["dxr"]) <= 1e-4, (rel(r["y"], r["yr"]), rel(r["dx"], r["dxr"]))
    pr = dict(r["ref"].named_parameters())
    for n, p in r["m"].named_parameters():
        assert rel(p.grad, pr[n].grad) <= 1e-4, (n, rel(p.grad, pr[n].grad))


@pytest.mark.parametrize("name", C.NAMES)
def test_the_reference_gets_its_settings(name):
    """state-dict keys and shapes of the restatement are the model's -- and a restatement built with the DEFAULT settings has other
    shapes: every row differs from the defaults in a parameter's shape, so a reference that silently ignored its settings fails here"""
    r = _run(name)
    sm, sr = r["m"].state_dict(), r["ref"].state_dict()
    assert list(sm) == list(sr)
    assert all(sm[k].shape == sr[k].shape for k in sm), [k for k in sm if sm[k].shape != sr[k].shape]
    c = C.CASES[name]
    sd = R.SegformerReference(c["cin"], c["cout"]).state_dict()
    assert set(sd) != set(sm) or any(sd[k].shape != sm[k].shape for k in sm)
    stage0 = r["ref"].mit.stages[0]
    assert stage0[2][0][0].fn.to_kv.weight.shape[-1] == c["reduction_ratio"][0] and len(stage0[2]) == c["num_layers"]


@pytest.mark.parametrize("name", C.NAMES)
def test_every_block_has_an_own_part_worth_checking(name):
    """the condition of the device's block checks (tests/test_segformer_nodes_gpu.py::check_block_nodes holds y - x to 3e-2 and needs
    |y - x| >= 0.05 |x|): in the float64 restatement alone, for every attention and Mix-FFN block of the row.  A condition on the
    seeds of tests/segformer_settings_cases.py, not a measurement of a kernel."""
    own = _run(name)["own"]
    assert len(own) == 8 * C.CASES[name]["num_layers"]
    assert min(own) >= 0.05, [f"{v:.3f}" for v in own]


# ------------------------------------------------------------------------------------------------ the node references against torch
def _close(a, b):
    return torch.allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("C_,D,k,s,p,hw", [(5, 8, 3, 2, 1, (8, 12)), (8, 32, 7, 4, 3, (16, 24)), (32, 64, 3, 2, 1, (6, 4)),
                                           (16, 24, 1, 1, 0, (3, 5))])
def test_patch_conv_reference(C_, D, k, s, p, hw):
    """against the network's own statement: nn.Unfold(k, s, p) + Conv2d(C k^2, D, 1) (the embeddings) and Conv2d(C, D, k, s, p) (the
    downsampler) with the same numbers -- the (D, C k^2) view is in Unfold's column order"""
    torch.manual_seed(k + C_)
    unfold, embed = nn.Unfold(k, stride=s, padding=p), nn.Conv2d(C_ * k * k, D, 1).double()
    x = torch.randn(2, C_, *hw, dtype=torch.float64, requires_grad=True)
    ho, wo = (hw[0] + 2 * p - k) // s + 1, (hw[1] + 2 * p - k) // s + 1
    y = embed(unfold(x).reshape(2, -1, ho, wo))
    conv = nn.Conv2d(C_, D, k, stride=s, padding=p).double()
    with torch.no_grad():
        conv.weight.copy_(embed.weight.view(D, C_, k, k))
        conv.bias.copy_(embed.bias)
    assert _close(conv(x), y)
    xl = x.detach().permute(0, 2, 3, 1).requires_grad_(True)
    w2d = embed.weight.view(D, -1)
    yn = N.patch_conv_ref(xl, w2d, embed.bias, k, s, p)
    assert _close(yn, y.permute(0, 2, 3, 1))
    dy = torch.randn_like(yn)
    gx, gw, gb = torch.autograd.grad(yn, (xl, embed.weight, embed.bias), dy)
    rx, rw, rb = torch.autograd.grad(y, (x, embed.weight, embed.bias), dy.permute(0, 3, 1, 2))
    assert _close(gx, rx.permute(0, 2, 3, 1)) and _close(gw, rw) and _close(gb, rb)


def _stage_maps(dims, hw, B=2):
    return [torch.randn(B, d, hw[0] >> i, hw[1] >> i, dtype=torch.float64, requires_grad=True) for i, d in enumerate(dims)]


def test_decoder_references():
    """linear_ref, up_sum_ref, decoder_cat_ref and decoder_sliced_ref against the modules of the restatement: to_fused (Conv2d 1x1 +
    nn.Upsample), torch.cat, to_segmentation -- and the column blocks matter: taking stage i's block for stage i + 1 moves the result by O(1)"""
    torch.manual_seed(2)
    dims, dd, O, hw = (8, 16, 24, 40), 16, 5, (16, 8)
    ref = R.SegformerReference(3, O, dims=dims, heads=(1, 1, 1, 1), decoder_dim=dd).double()
    feats = _stage_maps(dims, hw)
    fused_up = [tf(f) for f, tf in zip(feats, ref.to_fused)]
    seg0, seg1 = ref.to_segmentation
    mid = seg0(torch.cat(fused_up, dim=1))
    out = ref.upsample(seg1(mid))
    nl = [f.detach().permute(0, 2, 3, 1).requires_grad_(True) for f in feats]
    fused = [N.linear_ref(f, tf[0].weight.view(dd, -1), tf[0].bias) for f, tf in zip(nl, ref.to_fused)]
    for i, (a, b) in enumerate(zip(fused, fused_up)):       # (the module's map is the stage's own, repeated 2^i x 2^i)
        assert _close(a, b[..., ::2 ** i, ::2 ** i].permute(0, 2, 3, 1))
    mid_cat = N.decoder_cat_ref(fused, seg0.weight, seg0.bias)
    mid_sl = N.decoder_sliced_ref(fused, seg0.weight, seg0.bias)
    assert _close(mid_cat, mid.permute(0, 2, 3, 1)) and _close(mid_sl, mid.permute(0, 2, 3, 1))
    outn = N.upsample8_ref(N.linear_ref(mid_sl, seg1.weight.view(O, dd), seg1.bias))
    assert _close(outn, out.permute(0, 2, 3, 1))
    dy = torch.randn_like(outn)
    got = torch.autograd.grad(outn, nl + [seg0.weight, seg0.bias, seg1.weight], dy)
    want = torch.autograd.grad(out, feats + [seg0.weight, seg0.bias, seg1.weight], dy.permute(0, 3, 1, 2))
    for g, w in zip(got[:4], want[:4]):
        assert _close(g, w.permute(0, 2, 3, 1))
    assert all(_close(g, w) for g, w in zip(got[4:], want[4:]))
    # the slips a wrong decoder would make: the next stage's column block, or the bias once per stage
    w = seg0.weight.detach().view(dd, 4 * dd)
    fd = [f.detach() for f in fused]
    nxt = [(i + 1) % 4 for i in range(4)]
    shifted = N.up_sum_ref(*[N.linear_ref(f, w[:, j * dd: (j + 1) * dd], seg0.bias if i == 0 else None) for i, (f, j) in enumerate(zip(fd, nxt))])
    four_biases = N.up_sum_ref(*[N.linear_ref(f, w[:, i * dd: (i + 1) * dd], seg0.bias) for i, f in enumerate(fd)])
    assert rel(shifted, mid_cat) > 0.5 and rel(four_biases, mid_cat) > 3e-2


def test_up_sum_and_upsample_references():
    torch.manual_seed(3)
    zs = [torch.randn(2, 8 >> i, 16 >> i, 8, dtype=torch.float64, requires_grad=True) for i in range(4)]
    want = sum(nn.Upsample(scale_factor=2 ** i)(z.permute(0, 3, 1, 2)) for i, z in enumerate(zs)).permute(0, 2, 3, 1)
    got = N.up_sum_ref(*zs)
    assert _close(got, want)
    # the adjoint: 2^i x 2^i block sums
    dy = torch.randn_like(got)
    gz = torch.autograd.grad(got, zs, dy)
    for i, g in enumerate(gz):
        f = 2 ** i
        assert _close(g, dy.reshape(2, 8 // f, f, 16 // f, f, 8).sum(dim=(2, 4)))
    x = torch.randn(2, 3, 5, 8, dtype=torch.float64)
    up = nn.Upsample(scale_factor=8, mode="bilinear", align_corners=False)
    assert _close(N.upsample8_ref(x), up(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1))
    assert N.upsample8_ref(x).shape == (2, 24, 40, 8)


# ------------------------------------------------------------------------------------------------ the recorder and the refusals
def test_recorder_wraps_and_restores_the_module_level_names():
    from py4cast_amd import ops_gemm, ops_patch
    from py4cast_amd import segformer as S

    m = C.make_model("narrow", "bf16")
    before = (S.chan_layer_norm, S.sr_attention, S.patch_conv, S.up_sum, S.G)
    assert before[2] is ops_patch.patch_conv and before[4] is ops_gemm
    rec = N.Recorder(m)
    try:
        assert all(a is not b for a, b in zip(before, (S.chan_layer_norm, S.sr_attention, S.patch_conv, S.up_sum, S.G)))
        # the proxy overrides linear and upsample_add alone; the blocks' G.mlp and the nodes' G._f32 / GRADS_IN_PLACE are the module's own
        assert S.G.mlp is ops_gemm.mlp and S.G._f32 is ops_gemm._f32 and S.G.GRADS_IN_PLACE is ops_gemm.GRADS_IN_PLACE
        assert S.G.linear is not ops_gemm.linear and S.G.upsample_add is not ops_gemm.upsample_add
        assert ops_gemm.linear.__module__ == "py4cast_amd.ops_gemm"      # (the module itself is untouched: ops_patch keeps its own linear)
    finally:
        rec.undo()
    assert before == (S.chan_layer_norm, S.sr_attention, S.patch_conv, S.up_sum, S.G)
    assert "_attn" not in vars(m) or m._attn.__func__ is type(m)._attn
    assert (rec.blocks, rec.norms, rec.attns, rec.patch_convs, rec.linears, rec.up_sums, rec.upsamples) == ([],) * 7


def test_more_than_256_keys_refused_by_the_bf16_constructor_served_by_f32():
    from py4cast_amd.segformer import SegformerMI355X, SegformerSettings

    with pytest.raises(ValueError, match="384 at stage 1"):
        SegformerMI355X(8, 8, (128, 192), SegformerSettings(reduction_ratio=(1, 1, 1, 1), compute_dtype="bf16", activation_dtype="bf16"))
    SegformerMI355X(8, 8, None, SegformerSettings(reduction_ratio=(1, 1, 1, 1), compute_dtype="bf16", activation_dtype="bf16"))
    m = SegformerMI355X(8, 8, (128, 192), SegformerSettings(reduction_ratio=(1, 1, 1, 1)))
    with torch.no_grad():
        y = m(torch.randn(1, 128, 192, 8))
    assert y.shape == (1, 128, 192, 8) and bool(torch.isfinite(y).all())
