"""
The float64 node references of tests/unetrpp_nodes.py ARE the oracle's attention: composed by hand into the transformer block's
residual update t + gamma * EPA(x) -- the qkvv projection, the EPA core (``epa_node`` with its bf16 roundings off and E's weight
unrounded), the x_SA merge of either block form, the output projections with layer scale (``catlin_node``) -- forward, then backward
node by node in reverse, they must equal autograd of oracle/unetrpp.py::EPA in float64 within 1e-10: output, input gradient and every
parameter gradient, E = F included (the published block registers one Linear under both names; its gradient is counted once).  The
batch-norm reference equals conv51's tail with the published block's Dropout2d at a given draw, the passthrough gradient added to the
residual's.  Not composed here yet: the whole network (the convolution, group / instance norm and up-sampling references).  Runs on the
CPU.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import unetrpp_nodes as UN  # noqa: E402


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _unmerge(dm, B, H, N, d, published):
    """the adjoint of the x_SA merge (an exact permutation): (B, N, C) -> (B, heads, N, d)"""
    if published:
        return dm.reshape(B, d, H, N).permute(0, 2, 3, 1)
    return dm.reshape(B, N, H, d).permute(0, 2, 1, 3)


@pytest.mark.parametrize("published", [True, False])
@pytest.mark.parametrize("N,C,heads,p", [(64, 32, 4, 16), (48, 64, 8, 8), (32, 16, 1, 32)])
def test_epa_references_compose_to_the_oracle(published, N, C, heads, p):
    from oracle.unetrpp import EPA

    torch.manual_seed(N + C + heads + p + published)
    B, H, d = 2, heads, C // heads
    m = EPA(N, C, p, heads, published).double()
    with torch.no_grad():
        m.temperature.uniform_(0.5, 3.0)
        m.temperature2.uniform_(0.5, 3.0)
        m.E.bias.uniform_(-0.5, 0.5)
    if published:
        assert m.F is m.E
    gamma = (torch.rand(C, dtype=torch.float64) + 0.5).requires_grad_(True)
    x = torch.randn(B, N, C, dtype=torch.float64, requires_grad=True)
    r = torch.randn(B, N, C, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, N, C, dtype=torch.float64)
    y = r + gamma * m(x)
    y.backward(dy)
    params = dict(m.named_parameters())

    # forward through the node references
    Wq = m.qkvv.weight.detach()
    qkvv = (x.detach() @ Wq.t()).view(B, N, 4, H, d)
    e = UN.epa_node(qkvv, m.E.weight, m.E.bias, m.temperature, m.temperature2, rnd=False, round_weight=False)
    xa = UN.merge_published(e.x_sa) if published else UN.merge_restated(e.x_sa)
    xb = UN.merge_restated(e.x_ca)
    po, po2 = m.out_proj, m.out_proj2
    c = UN.catlin_node(xa, po.weight, po.bias, xb, po2.weight, po2.bias, r, gamma, dy=dy, round_weight=False)
    assert _rel(c.y, y.detach()) < 1e-10
    # backward, node by node in reverse
    e = UN.epa_node(qkvv, m.E.weight, m.E.bias, m.temperature, m.temperature2, dx_sa=_unmerge(c.dxa, B, H, N, d, published),
                    dx_ca=_unmerge(c.dxb, B, H, N, d, False), rnd=False, round_weight=False)
    dq = e.dqkvv.reshape(B * N, 4 * C)
    dx = (dq @ Wq).view(B, N, C)
    dWq = dq.t() @ x.detach().reshape(B * N, C)
    mine = {"qkvv.weight": dWq, "E.weight": e.dW, "E.bias": e.dbias, "temperature": e.dt1, "temperature2": e.dt2,
            "out_proj.weight": c.dwa, "out_proj.bias": c.dba, "out_proj2.weight": c.dwb, "out_proj2.bias": c.dbb}
    assert set(mine) == set(params), sorted(params)
    for n, g in mine.items():
        assert _rel(g, params[n].grad) < 1e-10, n
    assert _rel(dx, x.grad) < 1e-10
    assert _rel(c.dres, r.grad) < 1e-10
    assert _rel(c.dgamma, gamma.grad) < 1e-10


def test_epa_reference_roundings_are_the_named_ones():
    """rnd=True moves the outputs and gradients by about one bf16 rounding (of S, dL and the small matrices' images), never more;
    rnd=False is the oracle (above).  Guards a reference that silently stops rounding, or rounds far more than the docstring says."""
    torch.manual_seed(3)
    B, N, H, d, p = 2, 64, 4, 8, 16
    qkvv = torch.randn(B, N, 4, H, d, dtype=torch.float64)
    W, b = torch.randn(p, N, dtype=torch.float64) / 8, torch.rand(p, dtype=torch.float64) - 0.5
    t1, t2 = torch.rand(H, 1, 1, dtype=torch.float64) + 0.5, torch.rand(H, 1, 1, dtype=torch.float64) * 4 + 2
    dxs, dxc = torch.randn(B, H, N, d, dtype=torch.float64), torch.randn(B, H, N, d, dtype=torch.float64)
    ex = UN.epa_node(qkvv, W, b, t1, t2, dxs, dxc, rnd=False, round_weight=False)
    er = UN.epa_node(qkvv, W, b, t1, t2, dxs, dxc, rnd=True, round_weight=False)
    for a, bb in ((er.x_sa, ex.x_sa), (er.x_ca, ex.x_ca), (er.dqkvv, ex.dqkvv), (er.dW, ex.dW), (er.dbias, ex.dbias), (er.dt2, ex.dt2)):
        assert 0 < _rel(a, bb) < 4e-3


@pytest.mark.parametrize("with_mul", [True, False])
def test_bn_reference_is_conv51_tail_with_its_dropout(with_mul):
    """bn_act_node = the oracle's conv51 tail: leaky_relu(BatchNorm2d(y) + residual, 0.01), then the published block's Dropout2d with a
    given draw (mask per sample and channel, scaled by 1 / (1 - p)) -- output, gradients of y, the residual, gamma and beta, with the
    residual's passthrough gradient added -- against float64 autograd; and the running-statistics inputs (mean, unbiased variance)."""
    torch.manual_seed(5 + with_mul)
    B, H, W, C, p = 3, 4, 6, 8, 0.25
    y = torch.randn(B, H, W, C, dtype=torch.float64, requires_grad=True)
    res = torch.randn(B, H, W, C, dtype=torch.float64, requires_grad=True)
    bn = torch.nn.BatchNorm2d(C).double().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.3, 0.3)
    mul = (torch.rand(B, C) > p).float() if with_mul else None
    factor = 1 / (1 - p) if with_mul else 1.0
    dout, dpass = torch.randn(B, H, W, C, dtype=torch.float64), torch.randn(B, H, W, C, dtype=torch.float64)
    z = torch.nn.functional.leaky_relu(bn(y.permute(0, 3, 1, 2)) + res.permute(0, 3, 1, 2), 0.01)
    if with_mul:
        z = z * (mul.double() * factor)[:, :, None, None]           # Dropout2d's draw: one value per (sample, channel)
    out = z.permute(0, 2, 3, 1)
    out.backward(dout)
    ref = UN.bn_act_node(y, bn.weight, bn.bias, bn.eps, 0.01, res=res, mul=mul, factor=factor, dout=dout, dpass=dpass)
    assert _rel(ref.out, out.detach()) < 1e-12
    assert _rel(ref.dy, y.grad) < 1e-10 and _rel(ref.dgamma, bn.weight.grad) < 1e-10 and _rel(ref.dbeta, bn.bias.grad) < 1e-10
    assert _rel(ref.dres, res.grad + dpass) < 1e-10
    flat = y.detach().reshape(-1, C)
    assert _rel(ref.mean, flat.mean(0)) < 1e-12 and _rel(ref.var_unbiased, flat.var(0)) < 1e-12
    if with_mul:        # the draw belongs to its sample: swapping two samples' rows of the table moves the output
        swapped = UN.bn_act_node(y, bn.weight, bn.bias, bn.eps, 0.01, res=res, mul=mul.flip(0), factor=factor)
        assert _rel(swapped.out, out.detach()) > 1e-2
