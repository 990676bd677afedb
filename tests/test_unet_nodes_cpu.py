"""The float64 node references of tests/unet_nodes.py, composed into the whole UNet by hand (forward, then the backward node by node in
reverse, each node's decisions taken from this composition's own forward), against the autograd of the float64 restatement
(tests/unet_reference.py): the references the GPU node tests trust must BE the network, to rounding."""
import copy
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import unet_nodes as N  # noqa: E402
from unet_reference import UNetReference, padding_for  # noqa: E402


def rel(got, ref):
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def compose(ref, x, dy):
    """y, dx and {parameter name: gradient} of `ref` (train mode, float64) at x (B, H, W, Cin) for the output gradient dy, from the node
    references alone; and the per-norm BN results (for the running statistics)"""
    H, W = x.shape[1], x.shape[2]
    top, bottom, left, right = padding_for(H, W)
    h = F.pad(x, (0, 0, left, right, top, bottom))
    names = {id(p): n for n, p in ref.named_parameters()}
    grads, norms = {}, {}

    def put(p, g):
        grads[names[id(p)]] = g

    # ---- forward
    saved = {}
    for short, attr, _ in N.BLOCKS:
        seq = getattr(ref, attr)
        up_in = None
        if short.startswith("dec"):
            upm = getattr(ref, f"upconv{short[-1]}")
            up_in = h
            h = torch.cat((N.upconv_node(h, upm.weight, upm.bias, round_weight=False), saved[f"enc{short[-1]}"]["tail"].out), -1)
        c1 = N.conv_node(h, seq[0].weight, round_weight=False)
        b1 = N.bn_node(c1, seq[1].weight, seq[1].bias, seq[1].eps)
        c2 = N.conv_node(b1.out, seq[3].weight, round_weight=False)
        s = {"x": h, "c1": c1, "b1": b1, "c2": c2, "up_in": up_in}
        if short.startswith("enc"):
            s["tail"] = N.tail_node(c2, seq[4].weight, seq[4].bias, seq[4].eps)
            h = s["tail"].pool
        else:
            s["b2"] = N.bn_node(c2, seq[4].weight, seq[4].bias, seq[4].eps)
            h = s["b2"].out
        saved[short] = s
        norms[f"{attr}.{short}norm1"] = b1
        norms[f"{attr}.{short}norm2"] = s.get("b2", s.get("tail"))
    head_in = h
    y = N.conv_node(head_in, ref.conv.weight, ref.conv.bias, round_weight=False)
    # ---- backward, node by node in reverse
    dyp = F.pad(dy, (0, 0, left, right, top, bottom))
    _, dh, dw, db = N.conv_node(head_in, ref.conv.weight, ref.conv.bias, dy=dyp, round_weight=False)
    put(ref.conv.weight, dw)
    put(ref.conv.bias, db)
    dskip = {}
    for short, attr, _ in reversed(N.BLOCKS):
        seq = getattr(ref, attr)
        s = saved[short]
        if short.startswith("enc"):
            t = N.tail_node(s["c2"], seq[4].weight, seq[4].bias, seq[4].eps, act=s["tail"].out, dskip=dskip[short], dpool=dh)
            dc2, dg2, dbt2 = t.dy, t.dgamma, t.dbeta
        else:
            b2 = N.bn_node(s["c2"], seq[4].weight, seq[4].bias, seq[4].eps, mask=s["b2"].mask, dout=dh)
            dc2, dg2, dbt2 = b2.dy, b2.dgamma, b2.dbeta
        put(seq[4].weight, dg2)
        put(seq[4].bias, dbt2)
        _, db1, dw2, _ = N.conv_node(s["b1"].out, seq[3].weight, dy=dc2, round_weight=False)
        put(seq[3].weight, dw2)
        b1 = N.bn_node(s["c1"], seq[1].weight, seq[1].bias, seq[1].eps, mask=s["b1"].mask, dout=db1)
        put(seq[1].weight, b1.dgamma)
        put(seq[1].bias, b1.dbeta)
        _, dh, dw1, _ = N.conv_node(s["x"], seq[0].weight, dy=b1.dy, round_weight=False)
        put(seq[0].weight, dw1)
        if s["up_in"] is not None:
            upm = getattr(ref, f"upconv{short[-1]}")
            C = upm.weight.shape[1]
            dskip[f"enc{short[-1]}"] = dh[..., C:]
            _, dh, dwu, dbu = N.upconv_node(s["up_in"], upm.weight, upm.bias, dup=dh[..., :C], round_weight=False)
            put(upm.weight, dwu)
            put(upm.bias, dbu)
    crop = (slice(None), slice(top, top + H), slice(left, left + W))
    return y[crop], dh[crop], grads, norms


@pytest.mark.parametrize("hw,autopad", [((32, 48), False), ((30, 45), True)])
def test_node_references_compose_to_the_restatement(hw, autopad):
    torch.manual_seed(0)
    cin, cout, f = 5, 3, 8
    ref = UNetReference(cin, cout, f, autopad=autopad).double().train()
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
                m.running_mean.uniform_(-0.5, 0.5)
                m.running_var.uniform_(0.5, 2.0)
            elif getattr(m, "bias", None) is not None:
                m.bias.uniform_(-0.3, 0.3)
    pre = copy.deepcopy(ref)
    x = torch.randn(2, *hw, cin, dtype=torch.float64)
    dy = torch.randn(2, *hw, cout, dtype=torch.float64)
    y, dx, grads, norms = compose(ref, x, dy)
    xr = x.clone().requires_grad_(True)
    yr = ref(xr)
    yr.backward(dy)
    assert y.shape == yr.shape == (2, *hw, cout)
    assert rel(y, yr.detach()) <= 1e-10
    assert rel(dx, xr.grad) <= 1e-10
    params = dict(ref.named_parameters())
    assert set(grads) == set(params)
    for n, p in params.items():
        assert grads[n].shape == p.shape, n
        assert rel(grads[n], p.grad) <= 1e-10, n
    # the running statistics torch's BatchNorm2d keeps, from each node's batch statistics
    pmods, rmods = dict(pre.named_modules()), dict(ref.named_modules())
    assert len(norms) == 18
    for n, b in norms.items():
        rm, rv = N.running_update(pmods[n], b, rmods[n].momentum)
        assert rel(rm, rmods[n].running_mean) <= 1e-12 and rel(rv, rmods[n].running_var) <= 1e-12, n
