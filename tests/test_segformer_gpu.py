"""
Segformer (py4cast_amd/segformer.py) on the GPU: every kernel of csrc/segformer.hip against float64 torch on the same operands, the whole
network forward / backward against the float64 restatement (tests/segformer_reference.py) in both flavours, the native route of a bf16
step (no library convolution / GEMM / attention / norm / cat / interpolate; bit-identical reruns), HIP-graph replay against the eager
step, a scaled_ar rollout through the Lightning module and the reference's toy training loop.
Bars: bf16 kernels as tests/test_gemm_gpu.py (<= 6e-3 of the largest magnitude per element, <= 3e-3 in the 2-norm; the attention's
gradients 1e-2 in the 2-norm: dS = P (dP - D) subtracts two bf16-rounded products); fp32 parameter sums <= 5e-4; fp32 network 1e-4
relative; bf16 network: every activation is rounded to bf16 (2^-9 relative) through ~30 chained layers and 8 LayerNorms that divide by
per-pixel standard deviations -- 3e-2 on the output, and the gradients held to their direction (cosine) and 2-norm 1e-1.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from segformer_reference import SegformerReference, ref_forward_nhwc  # noqa: E402

pytestmark = pytest.mark.gpu


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def close_bf16(got, ref, what, worst_bar=6e-3, norm_bar=3e-3):
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    worst = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    assert worst <= worst_bar and rel(got, ref) <= norm_bar, f"{what}: max {worst:.2e}, 2-norm {rel(got, ref):.2e}"


def gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def bf(t):
    return t.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ spatial-reduction attention
@pytest.mark.parametrize("Nk,Nq,heads", [(1, 64, 1), (64, 4096, 1), (80, 5120, 1), (256, 64, 8), (64, 1024, 2), (80, 256, 5),
                                         (256, 4096, 2), (1, 5120, 8), (80, 64, 8), (64, 4096, 3),
                                         # off the default stages: masked tails of the 32-key chunk (3, 12, 31, 33, 255), whole chunks
                                         # only (192), one query, a partial query tile, up to the entry point's 64 heads
                                         (3, 1, 3), (12, 1536, 2), (31, 65, 1), (33, 63, 16), (192, 1536, 1), (255, 130, 10), (4, 64, 64)])
def test_sr_attention_against_float64(gpu_device, Nk, Nq, heads):
    from py4cast_amd.segformer import sr_attention

    dev = gpu_device
    g = gen(dev, Nk * 7 + Nq + heads)
    B, D = 2, 32 * heads
    q = bf(torch.randn(B, Nq, D, device=dev, generator=g))
    kv = bf(torch.randn(B, Nk, 2 * D, device=dev, generator=g))
    scale = 32 ** -0.5
    qg, kvg = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    out = sr_attention(qg, kvg, heads, scale)
    qd, kvd = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    qh = qd.view(B, Nq, heads, 32).transpose(1, 2)
    kh = kvd[..., :D].reshape(B, Nk, heads, 32).transpose(1, 2)
    vh = kvd[..., D:].reshape(B, Nk, heads, 32).transpose(1, 2)
    ref = ((qh @ kh.transpose(-1, -2)) * scale).softmax(-1) @ vh
    ref = ref.transpose(1, 2).reshape(B, Nq, D)
    close_bf16(out, ref, "out")
    dout = torch.randn(B, Nq, D, device=dev, generator=g)
    out.backward(bf(dout))
    ref.backward(bf(dout).double())
    close_bf16(qg.grad, qd.grad, "dq", 2e-2, 1e-2)
    close_bf16(kvg.grad, kvd.grad, "dkv", 2e-2, 1e-2)


# ------------------------------------------------------------------------------------------------ channel LayerNorm (std + eps)
@pytest.mark.parametrize("R,C", [(8192, 32), (2048, 64), (512, 160), (128, 256), (1000, 512),
                                 # one row; one partial lane fill (8, 96); 5 and 7.875 values per lane (320, 504: the widest partial fill)
                                 (1, 32), (257, 8), (130, 96), (67, 320), (33, 504)])
def test_chan_layer_norm_against_float64(gpu_device, R, C):
    from py4cast_amd.segformer import chan_layer_norm

    dev = gpu_device
    g = gen(dev, R + C)
    x = bf(torch.randn(R, C, device=dev, generator=g) * 2 + 0.5)
    gam = (1 + 0.3 * torch.randn(1, C, 1, 1, device=dev, generator=g)).requires_grad_(True)
    bet = (0.3 * torch.randn(1, C, 1, 1, device=dev, generator=g)).requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    y = chan_layer_norm(xg, gam, bet)
    xd = x.double().requires_grad_(True)
    gd, bd = gam.detach().double().requires_grad_(True), bet.detach().double().requires_grad_(True)
    sd = xd.var(-1, unbiased=False, keepdim=True).sqrt()
    yr = (xd - xd.mean(-1, keepdim=True)) / (sd + 1e-5) * gd.view(C) + bd.view(C)
    close_bf16(y, yr, "y")
    dy = bf(torch.randn(R, C, device=dev, generator=g))
    y.backward(dy)
    yr.backward(dy.double())
    close_bf16(xg.grad, xd.grad, "dx")
    assert rel(gam.grad, gd.grad) <= 5e-4 and rel(bet.grad, bd.grad) <= 5e-4
    # sums in a fixed order: a rerun is bit-identical
    g1, b1 = gam.grad.clone(), bet.grad.clone()
    gam.grad = bet.grad = None
    chan_layer_norm(x.clone().requires_grad_(True), gam, bet).backward(dy)
    assert torch.equal(gam.grad, g1) and torch.equal(bet.grad, b1)


# ------------------------------------------------------------------------------------------------ overlapping strided convolutions
@pytest.mark.parametrize("B,H,W,C,D,k,s,p", [(2, 128, 128, 8, 32, 3, 2, 1), (2, 64, 96, 32, 64, 7, 4, 3), (1, 32, 32, 64, 160, 3, 2, 1),
                                             (2, 64, 64, 32, 64, 8, 8, 0), (2, 16, 24, 160, 320, 2, 2, 0),
                                             # reduction ratio 1 (no gather: the GEMM alone) and 16 (one key per sample: a 2-row GEMM
                                             # over 16384 columns), the 7 x 7 embedding over 8 channels, ratio 1 at the widest dims
                                             (2, 8, 24, 32, 64, 1, 1, 0), (2, 16, 16, 64, 128, 16, 16, 0), (1, 32, 64, 8, 32, 7, 4, 3),
                                             (3, 4, 4, 512, 1024, 1, 1, 0)])
def test_patch_conv_against_float64(gpu_device, B, H, W, C, D, k, s, p):
    from py4cast_amd.segformer import patch_conv

    dev = gpu_device
    g = gen(dev, H + C + k)
    x = bf(torch.randn(B, H, W, C, device=dev, generator=g))
    w = (torch.randn(D, C, k, k, device=dev, generator=g) / (C * k * k) ** 0.5).requires_grad_(True)
    b = (0.1 * torch.randn(D, device=dev, generator=g)).requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    y = patch_conv(xg, w.view(D, -1), b, k, s, p)
    xd = x.double().requires_grad_(True)
    wd, bd = w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
    yr = F.conv2d(xd.permute(0, 3, 1, 2), wd, bd, stride=s, padding=p).permute(0, 2, 3, 1)
    close_bf16(y, yr, "y")
    dy = bf(torch.randn(yr.shape, device=dev, generator=g))
    y.backward(dy)
    yr.backward(dy.double())
    close_bf16(xg.grad, xd.grad, "dx")
    assert rel(w.grad, wd.grad) <= 5e-3 and rel(b.grad, bd.grad) <= 5e-3


# ------------------------------------------------------------------------------------------------ depthwise 3x3
@pytest.mark.parametrize("B,H,W,C", [(2, 64, 64, 256), (2, 32, 32, 512), (2, 16, 20, 640), (2, 8, 8, 1024), (1, 33, 7, 1024),
                                     # FFN widths of small expansions: one 8-channel group, less than one 512-channel block of the
                                     # weight gradient, and exactly one group in its second block (520)
                                     (2, 9, 7, 8), (2, 16, 12, 32), (1, 5, 33, 96), (2, 8, 8, 520)])
def test_depthwise_against_float64(gpu_device, B, H, W, C):
    from py4cast_amd.segformer import depthwise3x3

    dev = gpu_device
    g = gen(dev, H * W + C)
    x = bf(torch.randn(B, H, W, C, device=dev, generator=g))
    w = (torch.randn(C, 1, 3, 3, device=dev, generator=g) / 3).requires_grad_(True)
    b = (0.1 * torch.randn(C, device=dev, generator=g)).requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    y = depthwise3x3(xg, w, b)
    xd = x.double().requires_grad_(True)
    wd, bd = w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
    yr = F.conv2d(xd.permute(0, 3, 1, 2), wd, bd, padding=1, groups=C).permute(0, 2, 3, 1)
    close_bf16(y, yr, "y")
    dy = bf(torch.randn(yr.shape, device=dev, generator=g))
    y.backward(dy)
    yr.backward(dy.double())
    close_bf16(xg.grad, xd.grad, "dx")
    assert rel(w.grad, wd.grad) <= 5e-4 and rel(b.grad, bd.grad) <= 5e-4


# ------------------------------------------------------------------------------------------------ decoder up-sampling sum
@pytest.mark.parametrize("B,H,W,C", [(2, 64, 64, 256), (1, 8, 16, 8), (2, 64, 80, 64), (1, 8, 24, 64), (3, 16, 8, 128)])
def test_up_sum_against_float64(gpu_device, B, H, W, C):
    from py4cast_amd.segformer import up_sum

    dev = gpu_device
    g = gen(dev, H + W + C)
    zs = [bf(torch.randn(B, H >> i, W >> i, C, device=dev, generator=g)).requires_grad_(True) for i in range(4)]
    y = up_sum(*zs)
    zd = [z.detach().double().requires_grad_(True) for z in zs]
    yr = sum(F.interpolate(z.permute(0, 3, 1, 2), scale_factor=2 ** i, mode="nearest").permute(0, 2, 3, 1) for i, z in enumerate(zd))
    close_bf16(y, yr, "y")
    dy = bf(torch.randn(yr.shape, device=dev, generator=g))
    y.backward(dy)
    yr.backward(dy.double())
    for i in range(4):
        close_bf16(zs[i].grad, zd[i].grad, f"dz{i}")


# ------------------------------------------------------------------------------------------------ the network
def _pair(dev, cin, cout, dtype, seed=0, grid=(64, 64)):
    from py4cast_amd.segformer import SegformerMI355X, SegformerSettings

    torch.manual_seed(seed)
    key = "bf16" if dtype == torch.bfloat16 else "f32"
    m = SegformerMI355X(cin, cout, grid, SegformerSettings(compute_dtype=key, activation_dtype=key)).to(dev)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("norm.g") or n.endswith("norm.b"):
                p.add_(0.1 * torch.randn_like(p))
    ref = SegformerReference(cin, cout).to(dev).double()
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    return m, ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hw", [(64, 64), (128, 192), (512, 512)])
def test_network_against_restatement(gpu_device, dtype, hw):
    dev = gpu_device
    cin, cout = 69, 60
    m, ref = _pair(dev, cin, cout, dtype, grid=hw)
    g = gen(dev, 7)
    x = torch.randn(2, *hw, cin, device=dev, generator=g)
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    xd = x.double().requires_grad_(True)
    yr = ref_forward_nhwc(ref, xd)
    assert y.shape == yr.shape == (2, *hw, cout)
    dy = torch.randn(y.shape, device=dev, generator=g)
    y.float().backward(dy)
    yr.backward(dy.double())
    pr = dict(ref.named_parameters())
    if dtype == torch.float32:
        assert rel(y, yr) <= 1e-4
        assert rel(xg.grad, xd.grad) <= 1e-4
        for n, p in m.named_parameters():
            assert rel(p.grad, pr[n].grad) <= 1e-4, n
    else:
        assert rel(y, yr) <= 3e-2, rel(y, yr)
        assert rel(xg.grad, xd.grad) <= 1e-1, rel(xg.grad, xd.grad)
        rels = {n: rel(p.grad, pr[n].grad) for n, p in m.named_parameters()}
        assert max(rels.values()) <= 1e-1, max((v, n) for n, v in rels.items())
        flat = torch.cat([p.grad.double().flatten() for p in m.parameters()])
        flat_r = torch.cat([pr[n].grad.flatten() for n, _ in m.named_parameters()])
        assert float(F.cosine_similarity(flat, flat_r, dim=0)) >= 0.99


def test_grid_not_multiple_of_64_raises_in_forward(gpu_device):
    from py4cast_amd import _lib as L
    from py4cast_amd.segformer import SegformerMI355X, SegformerSettings

    m = SegformerMI355X(2, 1, None, SegformerSettings(compute_dtype="bf16")).to(gpu_device)
    with pytest.raises(L.P4CError):
        m(torch.randn(1, 96, 64, 2, device=gpu_device))


def test_toy_training_loop(gpu_device):
    """the reference's test_torch_training_loop semantics: in 2, out 1, 64 x 64, SGD, both flavours; finite losses, an eval-mode
    forward, and the fp32 parameters after the steps against the restatement's"""
    dev = gpu_device
    for dtype in (torch.float32, torch.bfloat16):
        m, ref = _pair(dev, 2, 1, dtype)
        opt = torch.optim.SGD(m.parameters(), lr=0.01)
        opt_r = torch.optim.SGD(ref.parameters(), lr=0.01)
        g = gen(dev, 3)
        for _ in range(3):
            x = torch.randn(4, 64, 64, 2, device=dev, generator=g)
            t = torch.randn(4, 64, 64, 1, device=dev, generator=g)
            for model, o, xx, tt, fwd in ((m, opt, x, t, m), (ref, opt_r, x.double(), t.double(), lambda v: ref_forward_nhwc(ref, v))):
                o.zero_grad()
                loss = F.mse_loss(fwd(xx).to(tt.dtype), tt)
                assert torch.isfinite(loss)
                loss.backward()
                o.step()
        m.eval()
        with torch.no_grad():
            y = m(torch.randn(1, 64, 64, 2, device=dev))
        assert y.shape == (1, 64, 64, 1) and torch.isfinite(y).all()
        pr = dict(ref.named_parameters())
        for n, p in m.named_parameters():
            assert rel(p, pr[n]) <= (1e-5 if dtype == torch.float32 else 1e-3), n


def test_native_route_bf16_step(gpu_device):
    from torch.profiler import ProfilerActivity, profile

    from py4cast_amd.segformer import SegformerMI355X, SegformerSettings

    dev = gpu_device
    torch.manual_seed(0)
    m = SegformerMI355X(69, 60, (128, 128), SegformerSettings(compute_dtype="bf16", activation_dtype="bf16")).to(dev)
    x = torch.randn(2, 128, 128, 72, device=dev).to(torch.bfloat16)
    x[..., 69:] = 0

    def step():
        m.zero_grad(set_to_none=True)
        y = m(x)
        y.float().square().mean().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), [p.grad.detach().clone() for p in m.parameters()]

    step()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        y1, g1 = step()
    names = [e.name for e in prof.events()]
    low = [n.lower() for n in names]
    for bad in ("miopen", "hipblaslt", "rocblas", "cijk_", "im2col", "col2im", "cat_", "catarray", "layer_norm", "softmax",
                "upsample_bilinear", "upsample_nearest", "scaled_dot_product", "flash", "efficient_attention"):
        hits = [n for n in low if bad in n and not n.startswith("p4c")]
        assert not hits, (bad, hits[:5])
    assert not [n for n in names if n in ("aten::cat", "aten::convolution", "aten::mm", "aten::addmm", "aten::bmm", "aten::baddbmm",
                                           "aten::matmul", "aten::einsum", "aten::cudnn_convolution", "aten::miopen_convolution",
                                           "aten::im2col", "aten::col2im", "aten::layer_norm", "aten::native_layer_norm", "aten::_softmax",
                                           "aten::scaled_dot_product_attention", "aten::upsample_nearest2d", "aten::upsample_bilinear2d",
                                           "aten::var", "aten::gelu")]
    y2, g2 = step()
    assert torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def _lm(dev, key, T=3, H=64, W=64, seed=72, strategy="scaled_ar"):
    from helpers import make_dataset_info, synthetic_case
    from py4cast_amd.lightning import AutoRegressiveLightning

    case = synthetic_case(seed=71, B=2, T=T, H=H, W=W, F=5, Ff=5, border=0)
    info = make_dataset_info(case, 5)
    torch.manual_seed(seed)
    lm = AutoRegressiveLightning({"compute_dtype": key, "activation_dtype": key}, info, None, num_input_steps=1, num_pred_steps_train=T,
                                 batch_size=2, model_name="Segformer",
                                 losses=[{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}],
                                 training_strategy=strategy).to(dev).train()
    return lm, case


def test_graph_replay_equals_eager_step(gpu_device):
    """trainer.GraphedTrainingStep on the bf16 route: the replay's loss and gradients are bit-identical to the eager step's"""
    from helpers import make_batch
    from py4cast_amd.trainer import FlatDDP, GraphedTrainingStep

    dev = gpu_device
    lm, case = _lm(dev, "bf16", T=2)
    ddp = FlatDDP(lm.model, 1)
    ddp.zero_grad()
    loss_e = lm.training_step(make_batch(case, dev), 0)
    loss_e.backward()
    loss_e = loss_e.detach().clone()
    eager = ddp.flat_grad.clone()
    ddp.zero_grad()
    step = GraphedTrainingStep(lm, make_batch(case, dev))
    ddp.zero_grad()
    loss_g = step(make_batch(case, dev))
    torch.cuda.synchronize()
    assert torch.equal(loss_g.float(), loss_e.float())
    assert torch.equal(ddp.flat_grad, eager)


@pytest.mark.parametrize("hw", [64, 128])
@pytest.mark.parametrize("key", ["f32", "bf16"])
def test_scaled_ar_rollout_through_lightning(gpu_device, key, hw):
    """``AutoRegressiveLightning(model_name="Segformer")``: 3-step scaled_ar rollout at 64 x 64 (one key per stage) and 128 x 128 (four),
    F = 5; loss and parameter gradients against the float64 restatement driven through the oracle rollout.  bf16: the rows come straight
    from build_x (bf16, zero-padded to the GEMM's 8-channel granularity)."""
    from helpers import make_batch
    from oracle import losses as olosses
    from oracle import rollout as orollout

    dev = gpu_device
    T = 3
    lm, case = _lm(dev, key, T=T, H=hw, W=hw)
    m = lm.model
    seen = []
    hook = m.register_forward_pre_hook(lambda mod, args: seen.append((args[0].dtype, args[0].shape[-1])))
    loss = lm.training_step(make_batch(case, dev), 0)
    loss.backward()
    hook.remove()
    if key == "bf16":
        assert m.rollout_input_format == (torch.bfloat16, (m.in_channels + 7) // 8 * 8)
        assert seen == [m.rollout_input_format] * T
    ref = SegformerReference(m.in_channels, m.out_channels).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in m.state_dict().items()})

    class Nhwc(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            return ref_forward_nhwc(self.inner, x)

    c = {k: (v.double() if v.is_floating_point() else v) for k, v in case.items()}
    statics = c["statics"].unsqueeze(0).expand(2, *c["statics"].shape)
    interior = 1.0 - c["border_mask"]
    pred = orollout.rollout(Nhwc(ref), c["inputs"], c["forcing"], c["outputs"], statics, c["border_mask"], interior, c["diff_std"],
                            c["diff_mean"], training_strategy="scaled_ar")
    wts = olosses.weighted_loss_weights(c["state_weight"], c["diff_std"], "mse")
    lref = olosses.weighted_loss(pred, c["outputs"], torch.ones_like(pred), wts, interior, "mse").mean()
    lref.backward()
    rg = dict(ref.named_parameters())
    if key == "f32":
        assert abs(loss.item() - lref.item()) / abs(lref.item()) < 2e-4
        worst = max((rel(p.grad.cpu(), rg[n].grad), n) for n, p in m.named_parameters())
        assert worst[0] < 1e-3, worst
    else:
        assert abs(loss.item() - lref.item()) / abs(lref.item()) < 2e-3
        # at 64 x 64 every stage has ONE key: the softmax is 1 whatever the query, and to_q gets no gradient (float64: rounding noise)
        top = max(float(rg[n].grad.norm()) for n, _ in m.named_parameters())
        live = {n for n, _ in m.named_parameters() if float(rg[n].grad.norm()) > 1e-9 * top}
        assert all(n.endswith("to_q.weight") for n, _ in m.named_parameters() if n not in live)
        cos = {n: float(F.cosine_similarity(p.grad.double().flatten().cpu(), rg[n].grad.flatten(), dim=0)) for n, p in m.named_parameters()
               if n in live}
        assert min(cos.values()) > 0.95, min((v, n) for n, v in cos.items())
