"""
Segformer node by node on the GPU (bf16 route): every channel LayerNorm, spatial-reduction attention core, attention block and Mix-FFN block
call of a network forward / backward, recorded with its operands (tests/segformer_nodes.py), against the float64 node references on the
same operands -- forward, and for the blocks the data and parameter gradients for the gradient the output received in the network's
backward.  Plus the production gradient route: parameter gradients ADDED into existing .grad buffers (pre-filled, and under FlatDDP).

Bars.  LayerNorm and attention core: one rounding of the output, the kernel bars of tests/test_gemm_gpu.py (6e-3 of the largest magnitude
per element, 3e-3 in the 2-norm).  Blocks: the output and dx hold the residual; they are held to 4e-3 / 1e-2 in the 2-norm as a whole,
and the block's own part (y - x, dx - dy) to 3e-2 -- it passes through 4 (attention) / 5 (Mix-FFN) bf16-stored intermediates, each
2^-9 relative, and the output's own rounding is relative to |x + branch|.  Parameter gradients (fp32 sums of bf16 operands) 3e-2.  The
attention block's to_q / to_kv: 1e-1 and a cosine >= 0.995 -- their gradients pass through dS = P (dP - D), and at initialisation the
logits are small, P is nearly uniform and dP - D is a small difference of two terms computed from bf16 q, k, v and o (measured up to
6.5e-2 at 512 x 512, stage 3).  A wiring error moves these by O(1).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import segformer_nodes as N  # noqa: E402

pytestmark = pytest.mark.gpu


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def close_bf16(got, ref, what, worst_bar=6e-3, norm_bar=3e-3):
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    worst = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    assert worst <= worst_bar and rel(got, ref) <= norm_bar, f"{what}: max {worst:.2e}, 2-norm {rel(got, ref):.2e}"


def _model(dev, hw, seed=0):
    from py4cast_amd.segformer import SegformerMI355X, SegformerSettings

    torch.manual_seed(seed)
    m = SegformerMI355X(69, 60, hw, SegformerSettings(compute_dtype="bf16", activation_dtype="bf16")).to(dev)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("norm.g") or n.endswith("norm.b"):
                p.add_(0.1 * torch.randn_like(p))
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    x = torch.randn(2, *hw, 72, device=dev, generator=g).to(torch.bfloat16)
    x[..., 69:] = 0
    dy = torch.randn(2, *hw, 60, device=dev, generator=g)
    return m, x, dy


@pytest.fixture(scope="module", params=[(128, 192), (512, 512)], ids=["128x192", "512x512"])
def recorded(request, gpu_device):
    m, x, dy = _model(gpu_device, request.param)
    rec = N.Recorder(m)
    try:
        y = m(x)
        y.float().backward(dy)
    finally:
        rec.undo()
    torch.cuda.synchronize()
    assert len(rec.blocks) == 16 and len(rec.norms) == 16 and len(rec.attns) == 8
    assert all(r["dy"] is not None for r in rec.blocks)
    return m, rec


# the checks themselves: also run on the non-default configurations of tests/test_segformer_settings_bf16_gpu.py, at the same bars
def check_layer_norm_nodes(rec):
    for i, r in enumerate(rec.norms):
        ref = N.ln(r["x"].double(), r["g"].double(), r["b"].double(), r["eps"])
        close_bf16(r["y"], ref, f"LayerNorm call {i}")


def check_sra_core_nodes(rec):
    for i, r in enumerate(rec.attns):
        ref = N.sra_core(r["q"].double(), r["kv"].double(), r["heads"], r["scale"])
        close_bf16(r["y"], ref, f"attention core call {i} (Nq {r['q'].shape[1]}, Nk {r['kv'].shape[1]}, heads {r['heads']})")


def check_block_nodes(m, rec, kind, count):
    orig = getattr(m, "_" + kind)
    calls = [r for r in rec.blocks if r["kind"] == kind]
    assert len(calls) == count
    for i, r in enumerate(calls):
        pn, x, dy = r["pn"], r["x"], r["dy"]
        what = f"{kind} block call {i} ({tuple(x.shape)})"
        # the native node alone on the recorded operands: the same output bit for bit, then its gradients for the recorded dy
        for p in pn.parameters():
            p.grad = None
        xl = x.clone().requires_grad_(True)
        y = orig(pn, xl)
        assert torch.equal(y, r["y"]), what
        y.backward(dy)
        names, leaves = N.block_params(kind, pn)
        x64 = x.double().requires_grad_(True)
        with torch.enable_grad():
            yr = N.block_ref(kind, pn, x64, leaves)
            grads = torch.autograd.grad(yr, [x64] + leaves, dy.double())
        x0 = x.double()
        assert rel(yr - x0, x0) >= 0.05, f"{what}: the block's own part is too small to check ({rel(yr - x0, x0):.2e})"
        assert rel(y, yr) <= 4e-3, f"{what}: y {rel(y, yr):.2e}"
        assert rel(y.double() - x0, yr - x0) <= 3e-2, f"{what}: y - x {rel(y.double() - x0, yr - x0):.2e}"
        dx, dxr, d0 = xl.grad.double(), grads[0], dy.double()
        assert rel(dx, dxr) <= 1e-2, f"{what}: dx {rel(dx, dxr):.2e}"
        assert rel(dx - d0, dxr - d0) <= 3e-2, f"{what}: dx - dy {rel(dx - d0, dxr - d0):.2e}"
        params = dict(pn.named_parameters())
        for n, gr in zip(names, grads[1:]):
            got = params[n].grad
            assert got is not None, f"{what}: {n} got no gradient"
            if n == "fn.to_q.weight" and r["pn"].fn.reduction_ratio ** 2 == x.shape[1] * x.shape[2]:
                # ONE key per sample: the softmax is 1 whatever the query, dS = P (dP - D) is zero term by term in float64 and in the
                # kernel alike (o = v, so dP and D are the same fp32 sum) -- no direction to compare: exact zeros on both sides
                assert not bool(gr.any()) and not bool(got.any()), f"{what}: {n} with one key: |got| {float(got.norm()):.2e}"
                continue
            if n in ("fn.to_q.weight", "fn.to_kv.weight"):
                cos = float(torch.nn.functional.cosine_similarity(got.double().flatten(), gr.flatten(), dim=0))
                assert rel(got, gr) <= 1e-1 and cos >= 0.995, f"{what}: {n} {rel(got, gr):.2e}, cosine {cos:.5f}"
            else:
                assert rel(got, gr) <= 3e-2, f"{what}: {n} {rel(got, gr):.2e}"


def test_layer_norm_nodes(recorded):
    check_layer_norm_nodes(recorded[1])


def test_sra_core_nodes(recorded):
    check_sra_core_nodes(recorded[1])


@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_block_nodes(recorded, kind):
    check_block_nodes(*recorded, kind, 8)


def check_sink_route(m, x, dy, gpu_device):
    """parameter gradients pre-filled (the GEMMs, LayerNorms and depthwise convolutions then ADD theirs into .grad in place; the decoder's
    weight slices, the padded downsampler and head go through autograd's accumulation), and under FlatDDP with a non-zero flat buffer:
    p.grad = prefill + the gradient of the .grad-is-None run, bit for bit"""
    from py4cast_amd.trainer import FlatDDP

    def step():
        m(x).float().backward(dy)
        torch.cuda.synchronize()

    m.zero_grad(set_to_none=True)
    step()
    g_none = {n: p.grad.clone() for n, p in m.named_parameters()}
    g = torch.Generator(device=gpu_device).manual_seed(11)
    prefill = {n: (torch.rand(p.shape, device=p.device, generator=g) + 0.5) * (1 - 2 * (torch.rand(p.shape, device=p.device, generator=g) < 0.5))
               for n, p in m.named_parameters()}
    for n, p in m.named_parameters():
        p.grad = prefill[n].clone()
    step()
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, prefill[n] + g_none[n]), f"prefilled .grad: {n}"
    ddp = FlatDDP(m, 1)
    for n, p in m.named_parameters():
        assert p.grad.data_ptr() >= ddp.flat_grad.data_ptr(), n
        p.grad.copy_(prefill[n])
    step()
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, prefill[n] + g_none[n]), f"FlatDDP .grad: {n}"


def test_sink_route_adds_into_grad(gpu_device):
    check_sink_route(*_model(gpu_device, (128, 128), seed=3), gpu_device)
