"""The float64 node references of tests/segformer_nodes.py against the modules of the network restatement (tests/segformer_reference.py):
the attention and Mix-FFN PreNorm blocks, NCHW modules against the features-last references, forward and gradients."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import segformer_nodes as N  # noqa: E402
import segformer_reference as R  # noqa: E402


def _randomise(mod):
    torch.manual_seed(5)
    with torch.no_grad():
        for p in mod.parameters():
            p.add_(0.2 * torch.randn_like(p))


@pytest.mark.parametrize("D,heads,r,hw", [(32, 1, 8, (16, 24)), (64, 2, 4, (8, 8)), (160, 5, 2, (4, 6)), (256, 8, 1, (2, 2))])
def test_attention_block_reference(D, heads, r, hw):
    blk = R.PreNorm(D, R.EfficientSelfAttention(dim=D, heads=heads, reduction_ratio=r)).double()
    _randomise(blk)
    x = torch.randn(2, D, *hw, dtype=torch.float64, requires_grad=True)
    y = blk(x) + x
    a = blk.fn
    xl = x.detach().permute(0, 2, 3, 1).requires_grad_(True)
    yn = N.attn_block(xl, blk.norm.g, blk.norm.b, blk.norm.eps, a.to_q.weight, a.to_kv.weight, a.to_out.weight, heads, r, a.scale)
    assert torch.allclose(yn, y.permute(0, 2, 3, 1), rtol=1e-10, atol=1e-10)
    dy = torch.randn_like(yn)
    gx, gw = torch.autograd.grad(yn, (xl, a.to_kv.weight), dy)
    rx, rw = torch.autograd.grad(y, (x, a.to_kv.weight), dy.permute(0, 3, 1, 2))
    assert torch.allclose(gx, rx.permute(0, 2, 3, 1), rtol=1e-10, atol=1e-10) and torch.allclose(gw, rw, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("D,f,hw", [(32, 8, (16, 8)), (160, 4, (4, 6))])
def test_mix_ffn_block_reference(D, f, hw):
    blk = R.PreNorm(D, R.MixFeedForward(dim=D, expansion_factor=f)).double()
    _randomise(blk)
    x = torch.randn(2, D, *hw, dtype=torch.float64, requires_grad=True)
    y = blk(x) + x
    fc1, ds, _, fc2 = blk.fn.net
    dw, pw = ds.net
    xl = x.detach().permute(0, 2, 3, 1).requires_grad_(True)
    yn = N.ff_block(xl, blk.norm.g, blk.norm.b, blk.norm.eps, fc1.weight, fc1.bias, dw.weight, dw.bias, pw.weight, pw.bias, fc2.weight, fc2.bias)
    assert torch.allclose(yn, y.permute(0, 2, 3, 1), rtol=1e-10, atol=1e-10)
    dy = torch.randn_like(yn)
    gx, gw = torch.autograd.grad(yn, (xl, dw.weight), dy)
    rx, rw = torch.autograd.grad(y, (x, dw.weight), dy.permute(0, 3, 1, 2))
    assert torch.allclose(gx, rx.permute(0, 2, 3, 1), rtol=1e-10, atol=1e-10) and torch.allclose(gw, rw, rtol=1e-10, atol=1e-10)


def test_block_params_follow_module_layout():
    from py4cast_amd.segformer import SegformerMI355X, SegformerSettings

    m = SegformerMI355X(4, 3, (64, 64), SegformerSettings())
    names = dict(m.named_parameters())
    attn, ff = m.mit.stages[1][2][0]
    for kind, pn, prefix in (("attn", attn, "mit.stages.1.2.0.0."), ("ff", ff, "mit.stages.1.2.0.1.")):
        got, leaves = N.block_params(kind, pn)
        assert sorted(prefix + n for n in got) == sorted(n for n in names if n.startswith(prefix))
        for n, t in zip(got, leaves):
            assert t.shape == names[prefix + n].shape
