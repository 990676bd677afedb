"""The deferred gradient reductions (py4cast_amd._lib.GradQueue; the ``defer`` argument of p4c_gemm_tn, p4c_row_mlp_bwd_accumulate and
p4c_node_proj_wgrad) after a backward pass that raised before the autograd engine ran its flush: the next pass -- with a gradient-sink
listener registered (what FlatDDP(overlap=True) does) or with the queue disabled -- adds every sum, reports a view only once its sum
has been added, and leaves nothing queued.  Both producer families: the accumulating gemm_tn calls of ops_gemm.linear, and
node_proj + row_mlp of the mesh GNNs."""

import pytest
import torch

pytestmark = pytest.mark.gpu


class _Boom(torch.autograd.Function):
    """identity; its backward raises -- applied to the input, it runs after the backward of every layer behind it"""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError("boom")


class _Snapshots:
    """a gradient-sink listener that keeps a copy, taken on the current stream, of every view reported as written"""

    def __init__(self):
        self.last = {}

    def sink_taken(self, view):
        pass

    def written(self, views):
        for v in views:
            self.last[(v.data_ptr(), tuple(v.shape), v.stride())] = (v, v.clone())


def _gemm_family(dev):
    from py4cast_amd import ops_gemm as G

    torch.manual_seed(81)
    lins = [torch.nn.Linear(128, 256).to(dev), torch.nn.Linear(256, 128).to(dev)]
    params = [p for m in lins for p in m.parameters()]

    def run(x):
        loss = 0.0
        for _ in range(2):      # two "AR steps" on the same weights
            h = G.linear(x, lins[0].weight, lins[0].bias)
            x = G.linear(h, lins[1].weight, lins[1].bias, res=x)
            loss = loss + x.float().square().mean()
        return loss

    return params, torch.randn(512, 128, device=dev).bfloat16(), run


def _gnn_family(dev):
    from py4cast_amd.ops_mlp import row_mlp
    from py4cast_amd.ops_nodeproj import node_proj

    torch.manual_seed(83)
    wide = (torch.randn(64, 192, device=dev) * 0.1).requires_grad_(True)
    aggr = (torch.randn(64, 128, device=dev) * 0.1).requires_grad_(True)
    b1, b2, beta = [(torch.randn(64, device=dev) * 0.1).requires_grad_(True) for _ in range(3)]
    w2 = (torch.randn(64, 64, device=dev) * 0.1).requires_grad_(True)
    gamma = (torch.rand(64, device=dev) + 0.5).requires_grad_(True)
    params = [wide, aggr, b1, w2, b2, gamma, beta]

    def run(h):
        loss = 0.0
        for _ in range(2):
            a, part = node_proj(h, [wide[:, 64:128], aggr[:, :64]])
            _, h = row_mlp(a, wide[:, :64], b1, w2, b2, gamma, beta, 1e-5, ga=part, res=h, want_out=False, grads_in_place=True)
            loss = loss + h.float().square().mean()
        return loss

    return params, torch.randn(1458, 64, device=dev).bfloat16(), run


@pytest.mark.parametrize("after", ["listener", "disabled"])
@pytest.mark.parametrize("family", ["gemm_tn", "node_proj"])
def test_a_backward_that_raised_leaves_no_stale_deferral(gpu_device, family, after):
    from py4cast_amd import _lib as L

    params, x0, run = (_gemm_family if family == "gemm_tn" else _gnn_family)(gpu_device)

    def backward(boom=False):
        for p in params:
            p.grad = torch.zeros_like(p)
        x = x0.clone().requires_grad_(True)
        run(_Boom.apply(x) if boom else x).backward()

    L.GradQueue.enabled = False
    try:
        backward()
    finally:
        L.GradQueue.enabled = True
    ref = [p.grad.clone() for p in params]

    with pytest.raises(RuntimeError, match="boom"):
        backward(boom=True)
    assert L.lib().p4c_grad_reduce_pending() > 0       # the dead pass left queued reductions behind

    snaps = _Snapshots()
    if after == "listener":
        L.GRAD_SINK_LISTENERS.append(snaps)
    else:
        L.GradQueue.enabled = False
    try:
        backward()
    finally:
        if snaps in L.GRAD_SINK_LISTENERS:
            L.GRAD_SINK_LISTENERS.remove(snaps)
        L.GradQueue.enabled = True
    torch.cuda.synchronize()
    if after == "listener":
        assert snaps.last
        for view, snap in snaps.last.values():
            assert torch.equal(snap, view), "a gradient view was reported written before its sum was added"
    for p, r in zip(params, ref):
        assert float(r.abs().max()) > 0 and torch.equal(p.grad, r)
    assert L.lib().p4c_grad_reduce_pending() == 0
