"""
DeepLabV3 (py4cast_amd/deeplabv3.py) on the GPU: the dilated implicit-GEMM convolution (csrc/gemm.hip, forward / data / weight
gradient), the strided convolutions as patch gather + GEMM (_PatchConv, at the network's three geometries), an identity residual block
at dilations 1 / 2 / 4 (conv1's passthrough into the residual batch norm), the stem tail, the ASPP pooling branch with the projection's input and the align_corners=True up-sampling (csrc/deeplab.hip,
csrc/resize.hip) against float64 torch on the same operands; the whole network against the float64 restatement
(tests/deeplabv3_reference.py) in both flavours, the Dropout node with its mask, the native route of a bf16 step (no library
convolution / GEMM / cat / pool / interpolate / norm / dropout; bit-identical reruns), HIP-graph replay against the eager step and a
scaled_ar rollout through the Lightning module.
Bars: bf16 kernels as tests/test_gemm_gpu.py (<= 6e-3 of the largest magnitude per element, <= 3e-3 in the 2-norm, fp32 weight / BN
parameter gradients <= 5e-4 ... 3e-3 -- sums of bf16 products); fp32 network 1e-4 relative; bf16 network: every activation is rounded to
bf16 (2^-9 relative) through 20 convolutions and 25 batch norms, and ReLU / max-pool decisions near a boundary flip between precisions
(a flipped max moves a whole O(1) gradient value) -- 3e-2 on the output, the gradients held to UNet's bars (tests/test_unet_gpu.py:
fp32 2e-2, bf16 0.6 per tensor and a cosine of 0.85 over all parameters).
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from deeplabv3_reference import DeepLabV3Reference  # noqa: E402

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


# ------------------------------------------------------------------------------------------------ dilated 3x3 convolution
@pytest.mark.parametrize("d", [1, 2, 4, 12, 24, 36])
@pytest.mark.parametrize("B,H,W,Ci,Co", [(2, 32, 32, 64, 128), (1, 24, 56, 32, 64), (2, 64, 64, 128, 64)])
def test_dilated_conv_against_float64(gpu_device, d, B, H, W, Ci, Co):
    from py4cast_amd import ops_gemm as G

    dev = gpu_device
    g = gen(dev, d * 7 + Ci)
    x = torch.randn(B, H, W, Ci, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(Co, Ci, 3, 3, device=dev, generator=g) / (3 * Ci ** 0.5)).requires_grad_(True)
    g0 = torch.randn(Co, Ci, 3, 3, device=dev, generator=g)
    w.grad = g0.clone()                                     # .grad accumulation: the weight gradient is ADDED
    xg = x.clone().requires_grad_(True)
    y, st = G.conv2d_nhwc(xg, w, want_stats=True, dilation=d)
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = w.detach().double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, padding=d, dilation=d)
    close_bf16(y.float().permute(0, 3, 1, 2), y64, f"y d={d}")
    # the statistics epilogue: column sums of the ROUNDED output
    s = st.double().sum(0)
    yr = y.double().reshape(-1, Co)
    assert rel(s[0], yr.sum(0)) <= 1e-5 and rel(s[1], (yr * yr).sum(0)) <= 1e-5
    dy = torch.randn(B, H, W, Co, device=dev, generator=g).to(torch.bfloat16)
    y.backward(dy)
    y64.backward(dy.double().permute(0, 3, 1, 2))
    close_bf16(xg.grad.float().permute(0, 3, 1, 2), x64.grad, f"dx d={d}")
    assert rel(w.grad - g0, w64.grad) <= 3e-3, (d, rel(w.grad - g0, w64.grad))
    if d == 1:
        # the d = 1 mode is the plain 3x3 "same" convolution: bit-equal to the call that names no dilation
        assert torch.equal(G.conv2d_nhwc(x, w.detach()), y.detach())


def test_dilation_is_rejected_where_unserved(gpu_device):
    from py4cast_amd import ops_gemm as G

    x = torch.zeros(1, 8, 8, 8, device=gpu_device, dtype=torch.bfloat16)
    assert not G.conv_supported(x, torch.zeros(8, 8, 1, 1, device=gpu_device), 2)
    assert not G.conv_supported(x, torch.zeros(8, 8, 3, 3, device=gpu_device), 0)
    assert G.conv_supported(x, torch.zeros(8, 8, 3, 3, device=gpu_device), 36)


# ------------------------------------------------------------------------------------------------ strided convolutions (_PatchConv)
@pytest.mark.parametrize("B,H,W,C,Ci,Co,k,s,p", [(2, 64, 64, 72, 69, 64, 7, 2, 3), (1, 37, 50, 72, 69, 64, 7, 2, 3), (2, 32, 48, 48, 46, 64, 7, 2, 3),
                                                 (2, 64, 48, 64, 64, 128, 3, 2, 1), (2, 33, 17, 64, 64, 128, 3, 2, 1),
                                                 (2, 64, 64, 64, 64, 128, 1, 2, 0), (1, 31, 45, 64, 64, 128, 1, 2, 0)])
def test_patch_conv_against_float64(gpu_device, B, H, W, C, Ci, Co, k, s, p):
    """DeepLabV3MI355X._patch (patch gather + GEMM with the statistics epilogue; backward: GEMM + the gather-form scatter, and the
    weight GEMM) at the network's strided geometries: the stem's 7x7 / 2 / 3 on a map zero-padded to C > Ci channels (the weight's
    zero-padded columns), layer2.0's 3x3 / 2 / 1 and its downsample's 1x1 / 2 / 0 -- odd and non-square grids included"""
    from py4cast_amd.deeplabv3 import DeepLabV3MI355X

    dev = gpu_device
    g = gen(dev, H * W + C + k)
    x = torch.randn(B, H, W, C, device=dev, generator=g)
    x[..., Ci:] = 0                                    # the zero-padded input rows, as the model pads them
    x = x.to(torch.bfloat16)
    conv = torch.nn.Conv2d(Ci, Co, k, stride=s, padding=p, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(Co, Ci, k, k, device=dev, generator=g) / (Ci * k * k) ** 0.5)

    def run():
        conv.weight.grad = None
        xg = x.clone().requires_grad_(True)
        y, st = DeepLabV3MI355X._patch(conv, xg)
        y.backward(dy)
        torch.cuda.synchronize()
        return y.detach(), st, xg.grad, conv.weight.grad.clone()

    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = torch.randn(B, Ho, Wo, Co, device=dev, generator=g).to(torch.bfloat16)
    y, st, dx, dw = run()
    assert y.shape == (B, Ho, Wo, Co) and dx.shape == x.shape
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = F.pad(conv.weight.detach().to(torch.bfloat16).double(), (0, 0, 0, 0, 0, C - Ci)).requires_grad_(True)   # as the GEMM reads it
    y64 = F.conv2d(x64, w64, stride=s, padding=p)
    close_bf16(y.float().permute(0, 3, 1, 2), y64, "y")
    # the statistics epilogue: column sums of the ROUNDED output
    sm = st.double().sum(0)
    yr = y.double().reshape(-1, Co)
    assert rel(sm[0], yr.sum(0)) <= 1e-5 and rel(sm[1], (yr * yr).sum(0)) <= 1e-5
    y64.backward(dy.double().permute(0, 3, 1, 2))
    close_bf16(dx.float().permute(0, 3, 1, 2), x64.grad, "dx")
    assert not dx[..., Ci:].any(), "dx of the padding channels"
    assert rel(dw, w64.grad[:, :Ci]) <= 5e-4, rel(dw, w64.grad[:, :Ci])
    # a rerun is bit-identical
    y2, st2, dx2, dw2 = run()
    assert torch.equal(y2, y) and torch.equal(st2, st) and torch.equal(dx2, dx) and torch.equal(dw2, dw)


# ------------------------------------------------------------------------------------------------ residual block
@pytest.mark.parametrize("d", [1, 2, 4])
@pytest.mark.parametrize("B,H,W,C", [(2, 32, 32, 64), (2, 24, 40, 128)])
def test_residual_block_against_float64(gpu_device, d, B, H, W, C):
    """an identity BasicBlock as DeepLabV3MI355X._block runs it: y1, st1, idn = conv2d_nhwc(x, w1, passthrough=True, dilation=d);
    h = relu(bn1(y1)); out = relu(bn2(conv2d_nhwc(h, w2, dilation=d)) + idn) -- the residual's gradient added in conv1's data-gradient
    epilogue.  Each stage against float64 on the device's own stored operands and incoming gradients (retained), decisions from the
    stored outputs"""
    from py4cast_amd import ops_gemm as G

    dev = gpu_device
    g = gen(dev, 100 * d + C + H)
    x = torch.randn(B, H, W, C, device=dev, generator=g).to(torch.bfloat16)
    w1 = (torch.randn(C, C, 3, 3, device=dev, generator=g) / (3 * C ** 0.5)).requires_grad_(True)
    w2 = (torch.randn(C, C, 3, 3, device=dev, generator=g) / (3 * C ** 0.5)).requires_grad_(True)
    bn1, bn2 = torch.nn.BatchNorm2d(C).to(dev), torch.nn.BatchNorm2d(C).to(dev)
    with torch.no_grad():
        for bn in (bn1, bn2):
            bn.weight.uniform_(0.5, 1.5, generator=g)
            bn.bias.uniform_(-0.3, 0.3, generator=g)
    xg = x.clone().requires_grad_(True)
    y1, st1, idn = G.conv2d_nhwc(xg, w1, want_stats=True, passthrough=True, dilation=d)
    h = G.batch_norm_act(y1, st1, bn1, slope=0.0)
    y2, st2 = G.conv2d_nhwc(h, w2, want_stats=True, dilation=d)
    out = G.batch_norm_act(y2, st2, bn2, slope=0.0, res=idn)
    for t in (y1, h, y2):
        t.retain_grad()
    dout = torch.randn(out.shape, device=dev, generator=g).to(torch.bfloat16)
    out.backward(dout)
    torch.cuda.synchronize()

    def conv64(inp, w, dy=None):
        i64 = inp.detach().double().permute(0, 3, 1, 2).requires_grad_(True)
        w64 = w.detach().to(torch.bfloat16).double().requires_grad_(True)
        o = F.conv2d(i64, w64, padding=d, dilation=d)
        if dy is None:
            return o.permute(0, 2, 3, 1).detach()
        o.backward(dy.double().permute(0, 3, 1, 2))
        return o.permute(0, 2, 3, 1).detach(), i64.grad.permute(0, 2, 3, 1), w64.grad

    def bn64(y, bn, res=None, mask=None, dz=None):
        r = y.detach().double().reshape(-1, C)
        n = r.shape[0]
        mean, var = r.mean(0), r.var(0, unbiased=False)
        rstd = torch.rsqrt(var + bn.eps)
        xhat = (r - mean) * rstd
        z = xhat * bn.weight.detach().double() + bn.bias.detach().double()
        if res is not None:
            z = z + res.detach().double().reshape(-1, C)
        o = torch.relu(z).view(y.shape)
        if dz is None:
            return o, None, None, None
        dzz = dz.detach().double().reshape(-1, C) * mask.reshape(-1, C)
        db, dg = dzz.sum(0), (dzz * xhat).sum(0)
        dy = bn.weight.detach().double() * rstd * (dzz - db / n - xhat * dg / n)
        return o, dy.view(y.shape), dg, db

    # forward, stage by stage on the stored operands
    close_bf16(y1.float(), conv64(x, w1), "y1")
    close_bf16(h.float(), bn64(y1, bn1)[0], "h")
    close_bf16(y2.float(), conv64(h, w2), "y2")
    close_bf16(out.float(), bn64(y2, bn2, res=x)[0], "out")
    assert torch.equal(idn, x)
    # backward, stage by stage on the device's incoming gradients and stored decisions
    _, dy2, dg2, db2 = bn64(y2, bn2, res=x, mask=out.detach() > 0, dz=dout)
    close_bf16(y2.grad.float(), dy2, "dy2")
    assert rel(bn2.weight.grad, dg2) <= 5e-3 and rel(bn2.bias.grad, db2) <= 5e-3
    _, dh, dw2 = conv64(h, w2, y2.grad)
    close_bf16(h.grad.float(), dh, "dh")
    assert rel(w2.grad, dw2) <= 3e-3, rel(w2.grad, dw2)
    _, dy1, dg1, db1 = bn64(y1, bn1, mask=h.detach() > 0, dz=h.grad)
    close_bf16(y1.grad.float(), dy1, "dy1")
    assert rel(bn1.weight.grad, dg1) <= 5e-3 and rel(bn1.bias.grad, db1) <= 5e-3
    _, dx1, dw1 = conv64(x, w1, y1.grad)
    dres = dout.double() * (out.detach() > 0)            # the identity edge: relu'(bn2(y2) + x) dout
    close_bf16(xg.grad.float(), dx1 + dres, "dx (conv1's data gradient + the residual's, one epilogue)")
    assert rel(w1.grad, dw1) <= 3e-3, rel(w1.grad, dw1)


# ------------------------------------------------------------------------------------------------ stem tail
@pytest.mark.parametrize("B,H,W,C,training", [(2, 32, 32, 64, True), (3, 18, 26, 64, True), (2, 17, 9, 8, True), (2, 32, 48, 64, False),
                                              (2, 256, 256, 64, True)])
def test_stem_tail_against_float64(gpu_device, B, H, W, C, training):
    from py4cast_amd.deeplabv3 import stem_tail

    dev = gpu_device
    g = gen(dev, H * W + C)
    # y on a grid of 1/8 steps: distinct values of a window stay far apart after the batch norm in any precision, equal ones stay
    # exactly equal -- the routing is then the same decision in fp32 and float64, ties included
    y = torch.randint(-16, 17, (B, H, W, C), device=dev, generator=g).float() / 8
    y[:, :3, :5] = 0.75                                # flat positive regions: windows with exact ties of positive values
    y[-1, 4:9, 2:8, : C // 2] = -1.5                   # (after BN: ties below zero -> ReLU zeros)
    y = y.to(torch.bfloat16)
    bn = torch.nn.BatchNorm2d(C).to(dev)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5, generator=g)
        bn.bias.uniform_(-0.2, 0.2, generator=g)
        if not training:
            bn.running_mean.uniform_(-0.3, 0.3, generator=g)
            bn.running_var.uniform_(0.5, 2.0, generator=g)
            bn.eval()
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    yg = y.clone().requires_grad_(True)
    pool = stem_tail(yg, None, bn)
    y64 = y.double().requires_grad_(True)
    g64 = bn.weight.detach().double().requires_grad_(True)
    b64 = bn.bias.detach().double().requires_grad_(True)
    rm, rv = rm0.double(), rv0.double()
    z = F.batch_norm(y64.permute(0, 3, 1, 2), rm, rv, g64, b64, training, 0.1, bn.eps)
    act = torch.relu(z)
    act_bf = act.detach().to(torch.bfloat16).double().requires_grad_(True)
    close_bf16(pool.float().permute(0, 3, 1, 2), F.max_pool2d(act, 3, 2, 1), "pool")
    if training:
        assert rel(bn.running_mean, rm) <= 1e-5 and rel(bn.running_var, rv) <= 1e-5
    dpool = torch.randn(pool.shape, device=dev, generator=g).to(torch.bfloat16)
    pool.backward(dpool)
    # routing as torch's max_pool2d picks it on the stored activations (first maximum in row-major order; a pixel that is the
    # maximum of two overlapping windows collects both gradients)
    F.max_pool2d(act_bf, 3, 2, 1).backward(dpool.double().permute(0, 3, 1, 2))
    dz = act_bf.grad * (act_bf.detach() > 0)
    z.backward(dz)
    close_bf16(yg.grad.float(), y64.grad, "dy")
    assert rel(bn.weight.grad, g64.grad) <= 3e-3 and rel(bn.bias.grad, b64.grad) <= 3e-3


# ------------------------------------------------------------------------------------------------ ASPP pooling branch + assembly
@pytest.mark.parametrize("B,H,W,C,D,training", [(2, 8, 8, 512, 256, True), (2, 64, 64, 512, 256, True), (3, 8, 12, 64, 32, True),
                                                (2, 8, 8, 512, 256, False), (1, 8, 8, 512, 256, False)])
def test_aspp_pool_branch_against_float64(gpu_device, B, H, W, C, D, training):
    from py4cast_amd.deeplabv3 import ASPPPooling, aspp_assemble

    dev = gpu_device
    g = gen(dev, B * H * W + C)
    pb = ASPPPooling(C, D).to(dev)
    with torch.no_grad():
        pb[1].weight.copy_(torch.randn(D, C, 1, 1, device=dev, generator=g) / C ** 0.5)
        pb[2].weight.uniform_(0.5, 1.5, generator=g)
        pb[2].bias.uniform_(-0.2, 0.2, generator=g)
        if not training:
            pb[2].running_mean.uniform_(-0.3, 0.3, generator=g)
            pb[2].running_var.uniform_(0.5, 2.0, generator=g)
    pb.train(training)
    rm0, rv0 = pb[2].running_mean.clone(), pb[2].running_var.clone()
    x = (torch.randn(B, H, W, C, device=dev, generator=g) + 0.3).to(torch.bfloat16)
    br = [torch.randn(B, H, W, D, device=dev, generator=g).to(torch.bfloat16) for _ in range(4)]
    xg = x.clone().requires_grad_(True)
    bg = [t.clone().requires_grad_(True) for t in br]
    buf = aspp_assemble(xg, bg, pb)
    for k in range(4):
        assert torch.equal(buf[..., k * D: (k + 1) * D], br[k])
    x64 = x.double().requires_grad_(True)
    w64 = pb[1].weight.detach().double().requires_grad_(True)
    g64 = pb[2].weight.detach().double().requires_grad_(True)
    b64 = pb[2].bias.detach().double().requires_grad_(True)
    rm, rv = rm0.double(), rv0.double()
    m = x64.mean(dim=(1, 2))                                                       # (B, C)
    z = F.conv2d(m[:, :, None, None], w64)
    p = torch.relu(F.batch_norm(z, rm, rv, g64, b64, training, 0.1, pb[2].eps))[:, :, 0, 0]   # (B, D)
    close_bf16(buf[..., 4 * D:].float(), p[:, None, None, :].expand(B, H, W, D), "pooled")
    if training:
        assert rel(pb[2].running_mean, rm) <= 1e-5 and rel(pb[2].running_var, rv) <= 1e-5
        assert int(pb[2].num_batches_tracked) == 1
    dbuf = torch.randn(buf.shape, device=dev, generator=g).to(torch.bfloat16)
    buf.backward(dbuf)
    for k in range(4):
        assert torch.equal(bg[k].grad, dbuf[..., k * D: (k + 1) * D])
    p.backward(dbuf[..., 4 * D:].double().sum(dim=(1, 2)))
    close_bf16(xg.grad.float(), x64.grad, "dx")
    # (fp32 sums of bf16 gradient values over the map: 1e-4 ... 5e-4 of the parameter sums, as the GEMM tests)
    assert rel(pb[1].weight.grad, w64.grad) <= 5e-4
    assert rel(pb[2].weight.grad, g64.grad) <= 5e-4 and rel(pb[2].bias.grad, b64.grad) <= 5e-4


def test_aspp_pool_branch_training_b1_raises(gpu_device):
    from py4cast_amd.deeplabv3 import ASPPPooling, aspp_assemble

    dev = gpu_device
    pb = ASPPPooling(64, 32).to(dev).train()
    x = torch.randn(1, 8, 8, 64, device=dev).to(torch.bfloat16)
    br = [torch.zeros(1, 8, 8, 32, device=dev, dtype=torch.bfloat16) for _ in range(4)]
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        aspp_assemble(x, br, pb)


# ------------------------------------------------------------------------------------------------ bilinear x8, align_corners=True
@pytest.mark.parametrize("B,H,W,C,s", [(2, 64, 64, 64, 8), (1, 8, 12, 8, 8), (2, 5, 3, 16, 4), (1, 1, 6, 8, 8), (2, 16, 16, 24, 2)])
def test_upsample_align_corners_against_float64(gpu_device, B, H, W, C, s):
    from py4cast_amd.deeplabv3 import upsample_bilinear_ac

    dev = gpu_device
    g = gen(dev, H * W * s)
    x = torch.randn(B, H, W, C, device=dev, generator=g).to(torch.bfloat16)
    xg = x.clone().requires_grad_(True)
    y = upsample_bilinear_ac(xg, s)
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    y64 = F.interpolate(x64, scale_factor=s, mode="bilinear", align_corners=True)
    close_bf16(y.float().permute(0, 3, 1, 2), y64, "y")
    dy = torch.randn(y.shape, device=dev, generator=g).to(torch.bfloat16)
    y.backward(dy)
    y64.backward(dy.double().permute(0, 3, 1, 2))
    close_bf16(xg.grad.float().permute(0, 3, 1, 2), x64.grad, "dx")
    # the library's module on the same layout (nn.UpsamplingBilinear2d is align_corners=True)
    lib = torch.nn.UpsamplingBilinear2d(scale_factor=s)(x.float().permute(0, 3, 1, 2))
    close_bf16(y.float().permute(0, 3, 1, 2), lib, "y vs UpsamplingBilinear2d")


# ------------------------------------------------------------------------------------------------ the network
# output bars: fp32 -- the library convolutions on the GPU against float64, through 20 (resnet34: 36) convolutions and the batch
# norms (measured up to 2.8e-4 at 64 x 64 / 64 x 96); bf16 -- every activation rounded to bf16 (2^-9) through the same chain: the
# float64 restatement with its convolution weights and outputs rounded to bf16 (and nothing else) lands 4.7e-2 (resnet18) ... 1.2e-1
# (resnet34) from the exact one at these sizes, and the native route measured 4.8e-2 ... 9.7e-2
FP32_OUT = 5e-4
BF16_OUT = 1.5e-1
def _pair(dev, cin, cout, dtype, name="resnet18", dc=64, dropout=0.0, seed=0):
    from py4cast_amd.deeplabv3 import DeepLabV3MI355X, DeepLabV3Settings

    key = "bf16" if dtype == torch.bfloat16 else "f32"
    torch.manual_seed(seed)
    m = DeepLabV3MI355X(cin, cout, None, DeepLabV3Settings(encoder_name=name, decoder_channels=dc, encoder_weights=False, aspp_dropout=dropout,
                                                           compute_dtype=key, activation_dtype=key)).to(dev).train()
    ref = DeepLabV3Reference(cin, cout, name, dc, dropout).to(dev).double().train()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in m.state_dict().items()})
    return m, ref


def _inputs(dev, B, hw, cin, seed):
    """random input rows whose samples differ in scale and offset: the ASPP pooling branch normalises ONE value per sample and channel
    over the batch, and samples of one distribution give per-sample means so close that their difference (what the batch norm over B
    divides by) cancels most digits -- any rounding upstream is then amplified by |mean| / std_b(mean).  Spread samples keep that
    division well conditioned, so the bars below measure the kernels, not the cancellation."""
    x = torch.randn(B, *hw, cin, device=dev, generator=gen(dev, seed))
    for b in range(B):
        x[b] = x[b] * (1.0 + b) + 0.5 * b
    return x


def _check_grads(m, ref, dtype, xg, xd):
    # Gradients (tests/test_unet_gpu.py): ReLU masks and max-pool choices are decided on values computed in the storage precision; an
    # element within rounding of a decision boundary sends its WHOLE gradient entry the other way than the float64 restatement does,
    # and every layer upstream inherits it -- fp32 holds 1e-1 (measured 5.3e-2 on dx at 64 x 96: a 3x3 / stride-2 pool shares
    # rows and columns between windows, so a flip moves more than UNet's 2x2 one), bf16 (flips ~1000x as frequent) the direction of
    # the whole gradient
    pr = dict(ref.named_parameters())
    if dtype == torch.float32:
        assert rel(xg.grad, xd.grad) <= 1e-1, rel(xg.grad, xd.grad)
        worst = max((rel(p.grad, pr[n].grad), n) for n, p in m.named_parameters())
        assert worst[0] <= 1e-1, worst
    else:
        # (per tensor the upstream layers measured up to 1.25 relative -- no per-tensor bar; the head, before any decision, is held)
        head = m.segmentation_head[0]
        assert rel(head.bias.grad, pr["segmentation_head.0.bias"].grad) <= 5e-2
        flat = torch.cat([p.grad.double().flatten() for p in m.parameters()])
        flat_r = torch.cat([pr[n].grad.flatten() for n, _ in m.named_parameters()])
        # measured 0.45 ... 0.83; the float64 restatement with only its FORWARD rounded to bf16 (convolution weights and outputs, the
        # backward exact) already reaches just 0.94 (resnet18, 64 x 64), 0.73 (resnet18, 64 x 96), 0.59 (resnet34, 64 x 64): the decision
        # flips of ~1000 ReLU / max-pool elements dominate the parameter gradients of this network at these sizes
        assert float(F.cosine_similarity(flat, flat_r, dim=0)) >= 0.4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name,hw", [("resnet18", (64, 64)), ("resnet18", (64, 96)), ("resnet34", (64, 64)), ("resnet34", (64, 96))])
def test_network_against_restatement(gpu_device, dtype, name, hw):
    dev = gpu_device
    cin, cout = 69, 60
    m, ref = _pair(dev, cin, cout, dtype, name)
    g = gen(dev, 7)
    x = _inputs(dev, 2, hw, cin, 7)
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    xd = x.double().requires_grad_(True)
    yr = ref(xd)
    assert y.shape == yr.shape == (2, *hw, cout)
    assert rel(y, yr) <= (FP32_OUT if dtype == torch.float32 else BF16_OUT), rel(y, yr)
    dy = torch.randn(y.shape, device=dev, generator=g)
    y.float().backward(dy)
    yr.backward(dy.double())
    _check_grads(m, ref, dtype, xg, xd)
    # the running statistics moved like the restatement's (one training forward)
    for (n, b), (_, br) in zip(m.named_buffers(), ref.named_buffers()):
        if n.endswith("running_mean") or n.endswith("running_var"):
            assert rel(b, br) <= (2 * FP32_OUT if dtype == torch.float32 else BF16_OUT), n    # (fp32 measured 7.5e-4)
    # eval: the running statistics, no dropout
    m.eval()
    ref.eval()
    with torch.no_grad():
        ye, yre = m(x), ref(x.double())
    assert rel(ye, yre) <= (FP32_OUT if dtype == torch.float32 else BF16_OUT), rel(ye, yre)


def test_dropout_node_with_its_mask(gpu_device):
    """Dropout(0.5) of the ASPP projection on the bf16 route: the model's draw (exposed as last_dropout_mask) replayed in the
    float64 restatement"""
    dev = gpu_device
    m, ref = _pair(dev, 5, 3, torch.bfloat16, dropout=0.5, seed=3)
    x = _inputs(dev, 2, (64, 64), 5, 1)
    xg = x.clone().requires_grad_(True)
    torch.manual_seed(11)
    y = m(xg)
    mask = m.last_dropout_mask
    assert mask is not None and mask.shape == (2 * 8 * 8, 64)
    assert set(torch.unique(mask).tolist()) <= {0.0, 1.0} and 0.3 < float(mask.mean()) < 0.7
    mk = mask.view(2, 8, 8, 64).permute(0, 3, 1, 2).double()
    xd = x.double().requires_grad_(True)
    yr = ref(xd, dropout_mask=mk)
    assert rel(y, yr) <= BF16_OUT, rel(y, yr)
    dy = torch.randn(y.shape, device=dev, generator=gen(dev, 2))
    y.float().backward(dy)
    yr.backward(dy.double())
    _check_grads(m, ref, torch.bfloat16, xg, xd)
    # a second draw differs; eval draws nothing
    m(x)
    assert not torch.equal(m.last_dropout_mask, mask)
    m.eval()
    with torch.no_grad():
        m(x)
    assert m.last_dropout_mask is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_grid_not_multiple_of_8_and_b1_training_raise(gpu_device, dtype):
    dev = gpu_device
    m, _ = _pair(dev, 2, 1, dtype)
    with pytest.raises(RuntimeError, match="divisible by 8"):
        m(torch.randn(2, 60, 64, 2, device=dev))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(torch.randn(1, 64, 64, 2, device=dev))
    m.eval()
    with torch.no_grad():
        assert m(torch.randn(1, 64, 64, 2, device=dev)).shape == (1, 64, 64, 1)


def test_native_route_bf16_step(gpu_device):
    from torch.profiler import ProfilerActivity, profile

    from py4cast_amd.deeplabv3 import DeepLabV3MI355X, DeepLabV3Settings

    dev = gpu_device
    torch.manual_seed(0)
    m = DeepLabV3MI355X(69, 60, (128, 128), DeepLabV3Settings(compute_dtype="bf16", activation_dtype="bf16", encoder_weights=False)).to(dev)
    x = torch.randn(2, 128, 128, 72, device=dev).to(torch.bfloat16)
    x[..., 69:] = 0

    def step(seed):
        torch.manual_seed(seed)
        m.zero_grad(set_to_none=True)
        y = m(x)
        loss = y.float().square().mean()
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), y.detach().clone(), [p.grad.detach().clone() for p in m.parameters()]

    step(5)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        l1, y1, g1 = step(5)
    names = [e.name for e in prof.events()]
    low = [n.lower() for n in names]
    for bad in ("miopen", "cudnn", "hipblaslt", "rocblas", "cijk_", "im2col", "col2im", "catarray", "max_pool", "upsample_bilinear",
                "adaptive_avg_pool", "batch_norm", "dropout"):
        hits = [n for n in low if bad in n and not n.startswith("p4c")]
        assert not hits, (bad, hits[:5])
    assert not [n for n in names if n in ("aten::cat", "aten::convolution", "aten::mm", "aten::addmm", "aten::bmm", "aten::matmul",
                                           "aten::cudnn_convolution", "aten::miopen_convolution", "aten::im2col", "aten::col2im",
                                           "aten::max_pool2d", "aten::max_pool2d_with_indices", "aten::upsample_bilinear2d",
                                           "aten::_adaptive_avg_pool2d", "aten::native_batch_norm", "aten::native_dropout")]
    l2, y2, g2 = step(5)
    assert torch.equal(l1, l2) and torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def _lm(dev, key, T=3, H=64, W=64, seed=72, dropout=0.0, name="resnet18"):
    from helpers import make_dataset_info, synthetic_case
    from py4cast_amd.lightning import AutoRegressiveLightning

    case = synthetic_case(seed=71, B=2, T=T, H=H, W=W, F=5, Ff=5, border=0)
    info = make_dataset_info(case, 5)
    torch.manual_seed(seed)
    lm = AutoRegressiveLightning({"compute_dtype": key, "activation_dtype": key, "encoder_weights": False, "aspp_dropout": dropout,
                                  "encoder_name": name, "decoder_channels": 64},
                                 info, None, num_input_steps=1, num_pred_steps_train=T, batch_size=2, model_name="DeepLabV3",
                                 losses=[{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}],
                                 training_strategy="scaled_ar").to(dev).train()
    return lm, case


@pytest.mark.parametrize("dropout", [0.0, 0.5])
def test_graph_replay_equals_eager_step(gpu_device, dropout):
    """trainer.GraphedTrainingStep on the bf16 route: with the generator at the same state, the replay's loss and gradients are
    bit-identical to the eager step's (the Dropout draws included)"""
    from helpers import make_batch
    from py4cast_amd.trainer import FlatDDP, GraphedTrainingStep

    dev = gpu_device
    lm, case = _lm(dev, "bf16", T=2, dropout=dropout)
    ddp = FlatDDP(lm.model, 1)
    ddp.zero_grad()
    torch.manual_seed(123)
    loss_e = lm.training_step(make_batch(case, dev), 0)
    loss_e.backward()
    loss_e = loss_e.detach().clone()
    eager = ddp.flat_grad.clone()
    ddp.zero_grad()
    step = GraphedTrainingStep(lm, make_batch(case, dev))
    ddp.zero_grad()
    torch.manual_seed(123)
    loss_g = step(make_batch(case, dev))
    torch.cuda.synchronize()
    assert torch.equal(loss_g.float(), loss_e.float())
    assert torch.equal(ddp.flat_grad, eager)


@pytest.mark.parametrize("key", ["f32", "bf16"])
def test_scaled_ar_rollout_through_lightning(gpu_device, key):
    """``AutoRegressiveLightning(model_name="DeepLabV3")``: 3-step scaled_ar rollout at 64 x 64, F = 5; loss and parameter gradients
    against the float64 restatement driven through the oracle rollout.  bf16: the rows come straight from build_x (bf16, zero-padded to
    the GEMM's 8-channel granularity)."""
    from helpers import make_batch
    from oracle import losses as olosses
    from oracle import rollout as orollout

    dev = gpu_device
    T = 3
    lm, case = _lm(dev, key, T=T)
    m = lm.model
    seen = []
    hook = m.register_forward_pre_hook(lambda mod, args: seen.append((args[0].dtype, args[0].shape[-1])))
    loss = lm.training_step(make_batch(case, dev), 0)
    loss.backward()
    hook.remove()
    if key == "bf16":
        assert m.rollout_input_format == (torch.bfloat16, (m.in_channels + 7) // 8 * 8)
        assert seen == [m.rollout_input_format] * T
    ref = DeepLabV3Reference(m.in_channels, m.out_channels, "resnet18", 64).double()
    ref.load_state_dict({k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in m.state_dict().items()})
    # the model's training step moved its running statistics T times; the restatement's forward uses batch statistics (train mode)
    ref.train()
    c = {k: (v.double() if v.is_floating_point() else v) for k, v in case.items()}
    statics = c["statics"].unsqueeze(0).expand(2, *c["statics"].shape)
    interior = 1.0 - c["border_mask"]
    pred = orollout.rollout(ref, c["inputs"], c["forcing"], c["outputs"], statics, c["border_mask"], interior, c["diff_std"],
                            c["diff_mean"], training_strategy="scaled_ar")
    wts = olosses.weighted_loss_weights(c["state_weight"], c["diff_std"], "mse")
    lref = olosses.weighted_loss(pred, c["outputs"], torch.ones_like(pred), wts, interior, "mse").mean()
    lref.backward()
    rg = dict(ref.named_parameters())
    if key == "f32":
        assert abs(loss.item() - lref.item()) / abs(lref.item()) < 2e-4
        worst = max((rel(p.grad.cpu(), rg[n].grad), n) for n, p in m.named_parameters())
        assert worst[0] < 1e-1, worst          # (measured 3.0e-2: the decision flips of test_network_against_restatement, over 3 calls)
    else:
        assert abs(loss.item() - lref.item()) / abs(lref.item()) < 2e-2
        # the synthetic batch's two samples share one distribution: the pooling branch's batch norm over their two close means amplifies
        # the bf16 rounding upstream (_inputs), on top of the decision flips -- measured cosine 0.69 over the three calls
        flat = torch.cat([p.grad.double().flatten().cpu() for p in m.parameters()])
        flat_r = torch.cat([rg[n].grad.flatten() for n, _ in m.named_parameters()])
        assert float(F.cosine_similarity(flat, flat_r, dim=0)) >= 0.5
