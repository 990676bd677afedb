"""
CustomUNet (py4cast_amd/customunet.py) on the GPU: the nearest-x2 + concatenation pass and the stem tail with its skip output
(csrc/customunet.hip) against torch on the same operands; the whole network against the restatement (tests/customunet_reference.py) in
both flavours, an autopad case, the native route of a bf16 step (no library convolution / GEMM / cat / pool / interpolate / norm;
bit-identical reruns), HIP-graph replay against the eager step and a diff_ar rollout through the Lightning module.
Bars (tests/test_deeplabv3_gpu.py's header): up2cat moves values, so its forward and dskip are bit-exact, and dx -- four bf16 values
added in fp32, rounded once -- lies within one bf16 rounding (half an ulp: 2^-8 relative) of the float64 sum; stem tail as DeepLabV3's
(<= 6e-3 of the largest magnitude per element, <= 3e-3 in the 2-norm, BN parameter gradients 3e-3); fp32 network 5e-4 on the output, 1e-1
on gradients (decision flips); bf16 network: see test_network_against_restatement.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from customunet_reference import CustomUNetReference, bf16_round_trip  # noqa: E402

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


# ------------------------------------------------------------------------------------------------ nearest x2 + concatenation
def _check_dx(dx, dout, Cx):
    """dx against the float64 sum of the four: half a bf16 ulp of the sum (2^-8 relative) + the three fp32 additions (2^-22 of the sum
    of magnitudes)"""
    B, H2, W2, _ = dout.shape
    d = dout[..., :Cx].double().view(B, H2 // 2, 2, W2 // 2, 2, Cx)
    s = d.sum(dim=(2, 4))
    mag = d.abs().sum(dim=(2, 4))
    err = (dx.double() - s).abs()
    assert bool((err <= 2.0 ** -8 * s.abs() + 2.0 ** -22 * mag).all()), float((err / s.abs().clamp_min(1e-30)).max())


@pytest.mark.parametrize("B,h,w,Cx,Cs", [(1, 1, 1, 8, 8), (2, 3, 5, 8, 16), (2, 17, 9, 24, 40), (2, 16, 16, 512, 256), (2, 96, 96, 128, 128)])
def test_up2cat_against_torch(gpu_device, B, h, w, Cx, Cs):
    """launch geometry (csrc/customunet.hip): a thread moves one 8-channel octet of one input pixel's 2x2 output block, 256 threads per
    workgroup, at most 2048 workgroups -- one pass of the grid-stride loop covers 524288 octets.  (2, 96, 96, 128, 128) has
    2 * 96 * 96 * 32 = 589824: the loop takes a second trip; (2, 16, 16, 512, 256) is decoder block 0 at 512 x 512, the widest rows."""
    from py4cast_amd.customunet import up2_cat

    dev = gpu_device
    g = gen(dev, h * w + Cx)
    x = torch.randn(B, h, w, Cx, device=dev, generator=g).to(torch.bfloat16)
    skip = torch.randn(B, 2 * h, 2 * w, Cs, device=dev, generator=g).to(torch.bfloat16)
    xg, sg = x.clone().requires_grad_(True), skip.clone().requires_grad_(True)
    out = up2_cat(xg, sg)
    want = torch.cat([F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), skip.permute(0, 3, 1, 2)], dim=1)
    assert torch.equal(out.detach(), want.permute(0, 2, 3, 1))
    dout = torch.randn(out.shape, device=dev, generator=g).to(torch.bfloat16)
    out.backward(dout)
    assert torch.equal(sg.grad, dout[..., Cx:])
    _check_dx(xg.grad, dout, Cx)


@pytest.mark.parametrize("B,h,w,Cx", [(2, 32, 48, 32), (2, 256, 256, 32)])
def test_up2cat_without_skip(gpu_device, B, h, w, Cx):
    """(2, 256, 256, 32): decoder block 4 of the 512 x 512 bench step -- 524288 octets, a grid exactly at the cap of 2048 workgroups
    with a full last workgroup and no second trip"""
    from py4cast_amd.customunet import up2_cat

    dev = gpu_device
    if h == 256:
        assert B * h * w * (Cx // 8) == 524288 == 2048 * 256
    g = gen(dev, 5)
    x = torch.randn(B, h, w, Cx, device=dev, generator=g).to(torch.bfloat16)
    xg = x.clone().requires_grad_(True)
    out = up2_cat(xg, None)
    assert out.shape == (B, 2 * h, 2 * w, Cx) and out.stride(2) == Cx
    assert torch.equal(out.detach(), F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1))
    dout = torch.randn(out.shape, device=dev, generator=g).to(torch.bfloat16)
    out.backward(dout)
    _check_dx(xg.grad, dout, Cx)


def test_up2cat_into_a_buffer_keeps_the_other_channels(gpu_device):
    """skip = None at ld = 128 > Cx = 64: the channels from Cx on keep what their producer wrote (a sentinel here), forward; the
    backward reads the first Cx channels of the buffer's gradient and hands the gradient on as it is"""
    from py4cast_amd.customunet import up2_into

    dev = gpu_device
    B, h, w, Cx, ld = 2, 9, 7, 64, 128
    g = gen(dev, 6)
    x = torch.randn(B, h, w, Cx, device=dev, generator=g).to(torch.bfloat16)
    xg = x.clone().requires_grad_(True)
    base = torch.full((B, 2 * h, 2 * w, ld), -7.5, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    buf = base * 1                                     # (a non-leaf the in-place node may write)
    out = up2_into(xg, buf)
    assert out.data_ptr() == buf.data_ptr()
    assert torch.equal(out.detach()[..., :Cx], F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1))
    assert bool((out.detach()[..., Cx:] == -7.5).all())
    dout = torch.randn(out.shape, device=dev, generator=g).to(torch.bfloat16)
    out.backward(dout)
    _check_dx(xg.grad, dout, Cx)
    assert torch.equal(base.grad[..., Cx:], dout[..., Cx:])


def test_up2cat_rejects_what_it_does_not_serve(gpu_device):
    from py4cast_amd._lib import P4CError
    from py4cast_amd.customunet import up2_cat

    dev = gpu_device
    x = torch.zeros(1, 4, 4, 8, device=dev, dtype=torch.bfloat16)
    with pytest.raises(P4CError):
        up2_cat(x[..., :4], None)                                                      # Cx off the 8-channel granularity
    with pytest.raises(P4CError):
        up2_cat(x, torch.zeros(1, 8, 9, 8, device=dev, dtype=torch.bfloat16))          # not the x2 grid
    with pytest.raises(P4CError):
        up2_cat(x.float(), None)


# ------------------------------------------------------------------------------------------------ stem tail with the skip
@pytest.mark.parametrize("B,H,W,C,training", [(2, 32, 32, 64, True), (3, 18, 26, 64, True), (2, 17, 9, 8, True), (2, 32, 48, 64, False),
                                              (2, 256, 256, 64, True)])
def test_stem_tail_skip_against_float64(gpu_device, B, H, W, C, training):
    """tests/test_deeplabv3_gpu.py::test_stem_tail_against_float64 with the activated map as a second output at a channel offset, and
    its gradient (dskip != 0) added to the routed pool gradient"""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops_gemm as G
    from py4cast_amd.customunet import stem_tail_skip

    dev = gpu_device
    g = gen(dev, H * W + C)
    off = 64 if C == 64 else 16
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
    buf, pool = stem_tail_skip(yg, None, bn, off)
    assert buf.shape == (B, H, W, off + C)
    y64 = y.double().requires_grad_(True)
    g64 = bn.weight.detach().double().requires_grad_(True)
    b64 = bn.bias.detach().double().requires_grad_(True)
    rm, rv = rm0.double(), rv0.double()
    z = F.batch_norm(y64.permute(0, 3, 1, 2), rm, rv, g64, b64, training, 0.1, bn.eps)
    act = torch.relu(z)
    act_bf = act.detach().to(torch.bfloat16).double().requires_grad_(True)
    close_bf16(buf[..., off:].float().permute(0, 3, 1, 2), act, "skip")
    close_bf16(pool.float().permute(0, 3, 1, 2), F.max_pool2d(act, 3, 2, 1), "pool")
    # the pool is the maximum of the STORED skip values, bit for bit
    assert torch.equal(pool.detach().permute(0, 3, 1, 2), F.max_pool2d(buf.detach()[..., off:].float().permute(0, 3, 1, 2), 3, 2, 1).to(torch.bfloat16))
    if training:
        assert rel(bn.running_mean, rm) <= 1e-5 and rel(bn.running_var, rv) <= 1e-5
    dpool = torch.randn(pool.shape, device=dev, generator=g).to(torch.bfloat16)
    dbuf = torch.randn(buf.shape, device=dev, generator=g).to(torch.bfloat16)      # (its first `off` channels are not the stem's to read)
    torch.autograd.backward([buf, pool], [dbuf, dpool])
    # routing as torch's max_pool2d picks it on the stored activations (first maximum in row-major order; a pixel that is the
    # maximum of two overlapping windows collects both gradients), plus the skip's own gradient
    F.max_pool2d(act_bf, 3, 2, 1).backward(dpool.double().permute(0, 3, 1, 2))
    dz = (act_bf.grad + dbuf[..., off:].double().permute(0, 3, 1, 2)) * (act_bf.detach() > 0)
    z.backward(dz)
    close_bf16(yg.grad.float(), y64.grad, "dy")
    assert rel(bn.weight.grad, g64.grad) <= 3e-3 and rel(bn.bias.grad, b64.grad) <= 3e-3
    # the entry point itself into a wider, sentinel-filled buffer at a channel offset: only channels [off, off + C) are written
    ld = off + C + 8
    wide = torch.full((B, H, W, ld), -7.5, device=dev, dtype=torch.bfloat16)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pool2 = torch.empty(B, Ho, Wo, C, device=dev, dtype=torch.bfloat16)
    arg = torch.empty(B, Ho, Wo, C, device=dev, dtype=torch.uint8)
    with torch.no_grad():
        st = G.bn_statistics(y, None, bn, False) if not training else None
    if st is None:      # the batch statistics again, without moving the running ones a second time
        r = y.float().reshape(-1, C)
        mean, var = r.mean(0), r.var(0, unbiased=False)
        scale = bn.weight.detach() * torch.rsqrt(var + bn.eps)
        st = torch.stack([mean, torch.rsqrt(var + bn.eps), scale, bn.bias.detach() - mean * scale]).contiguous()
    L.call("p4c_customunet_stem_fwd", L.ptr(y), L.ptr(st[2]), L.ptr(st[3]), L.ptr(wide[..., off:]), ld, L.ptr(pool2), L.ptr(arg), B, H, W, C,
           L.stream(dev))
    torch.cuda.synchronize()
    assert bool((wide[..., :off] == -7.5).all()) and bool((wide[..., off + C:] == -7.5).all())
    close_bf16(wide[..., off: off + C].float().permute(0, 3, 1, 2), act, "skip at an offset")
    assert int(arg.max()) <= 8


# ------------------------------------------------------------------------------------------------ the network
FP32_OUT = 5e-4
BF16_OUT = 1.5e-1         # tests/test_deeplabv3_gpu.py's bars: output, head-bias gradient, cosine over all parameter gradients
BF16_HEAD = 5e-2
BF16_COS = 0.4


def _pair(dev, cin, cout, dtype, name="resnet18", autopad=False, seed=0):
    from py4cast_amd.customunet import CustomUNetMI355X, CustomUNetSettings

    key = "bf16" if dtype == torch.bfloat16 else "f32"
    torch.manual_seed(seed)
    m = CustomUNetMI355X(cin, cout, None, CustomUNetSettings(encoder_name=name, encoder_weights=False, autopad_enabled=autopad,
                                                             compute_dtype=key, activation_dtype=key)).to(dev).train()
    ref = CustomUNetReference(cin, cout, name, autopad=autopad).to(dev).double().train()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in m.state_dict().items()})
    return m, ref


def _flat_grads(named):
    return torch.cat([p.grad.double().flatten() for _, p in named])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name,hw", [("resnet18", (64, 64)), ("resnet18", (64, 96)), ("resnet34", (64, 64)), ("resnet34", (64, 96))])
def test_network_against_restatement(gpu_device, dtype, name, hw):
    """both flavours against the float64 restatement on the same weights and inputs, training forward + backward, then eval.
    fp32 (library operations): output 5e-4, gradients 1e-1 (ReLU / max-pool decisions near a boundary flip between precisions) --
    measured: output 1.7e-5 ... 3.9e-5, input gradient 1.2e-2 ... 2.8e-2, worst parameter gradient 1.6e-2 ... 3.8e-2.
    bf16 (the native route): DeepLabV3's bars hold for this deeper network (31 convolutions; resnet34: 47) -- measured (resnet18 64 x 64,
    64 x 96, resnet34 64 x 64, 64 x 96): output 6.3e-2, 5.9e-2, 1.1e-1, 1.2e-1 of 1.5e-1; head-bias gradient 2.0e-3 of 5e-2; cosine over
    all parameter gradients 0.81, 0.82, 0.61, 0.54 of 0.4.  For scale, bf16 STORAGE alone (test_restatement_bf16_storage_error: the
    float64 restatement with every stored activation round-tripped through bf16, no kernel of this package) costs output 5.7e-2, 5.3e-2,
    9.9e-2, 1.1e-1 and cosine 0.79, 0.83, 0.70, 0.60 on the same inputs: the native route's distance is the storage format's."""
    dev = gpu_device
    cin, cout = 69, 60
    m, ref = _pair(dev, cin, cout, dtype, name)
    g = gen(dev, 7)
    x = torch.randn(2, *hw, cin, device=dev, generator=g)
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    xd = x.double().requires_grad_(True)
    yr = ref(xd)
    assert y.shape == yr.shape == (2, *hw, cout)
    dy = torch.randn(y.shape, device=dev, generator=g)
    y.float().backward(dy)
    yr.backward(dy.double())
    pr = dict(ref.named_parameters())
    head_b = rel(m.segmentation_head[0].bias.grad, pr["segmentation_head.0.bias"].grad)
    flat_r = torch.cat([pr[n].grad.flatten() for n, _ in m.named_parameters()])
    cos = float(F.cosine_similarity(_flat_grads(m.named_parameters()), flat_r, dim=0))
    print(f"\n{name} {hw} {dtype}: out {rel(y, yr):.3e} head-bias grad {head_b:.3e} cosine {cos:.4f} dx {rel(xg.grad, xd.grad):.3e}")
    if dtype == torch.float32:
        assert rel(y, yr) <= FP32_OUT, rel(y, yr)
        assert rel(xg.grad, xd.grad) <= 1e-1, rel(xg.grad, xd.grad)
        worst = max((rel(p.grad, pr[n].grad), n) for n, p in m.named_parameters())
        print(f"worst parameter gradient {worst}")
        assert worst[0] <= 1e-1, worst
    else:
        assert rel(y, yr) <= BF16_OUT, rel(y, yr)
        assert head_b <= BF16_HEAD, head_b
        assert cos >= BF16_COS, cos
    for (n, b), (_, br) in zip(m.named_buffers(), ref.named_buffers()):
        if n.endswith("running_mean") or n.endswith("running_var"):
            assert rel(b, br) <= (2 * FP32_OUT if dtype == torch.float32 else BF16_OUT), (n, rel(b, br))
    m.eval()
    ref.eval()
    with torch.no_grad():
        ye, yre = m(x), ref(x.double())
    print(f"eval out {rel(ye, yre):.3e}")
    assert rel(ye, yre) <= (FP32_OUT if dtype == torch.float32 else BF16_OUT), rel(ye, yre)


@pytest.mark.parametrize("name,hw", [("resnet18", (64, 64)), ("resnet18", (64, 96)), ("resnet34", (64, 64)), ("resnet34", (64, 96))])
def test_restatement_bf16_storage_error(gpu_device, name, hw):
    """what bf16 STORAGE alone costs this network: the float64 restatement with every stored activation round-tripped through bf16
    against the plain float64 one, same inputs and weights as test_network_against_restatement -- no kernel of this package runs.
    Printed for the record; the only assertion is that the two differ at the size bf16 predicts (above fp32's, below O(1))."""
    dev = gpu_device
    cin, cout = 69, 60
    _, ref = _pair(dev, cin, cout, torch.float32, name)
    rt = CustomUNetReference(cin, cout, name, round_trip=bf16_round_trip).to(dev).double().train()
    rt.load_state_dict(ref.state_dict())
    g = gen(dev, 7)
    x = torch.randn(2, *hw, cin, device=dev, generator=g)
    xa, xb = x.double().requires_grad_(True), x.double().requires_grad_(True)
    ya, yb = ref(xa), rt(xb)
    dy = torch.randn(ya.shape, device=dev, generator=g).double()
    ya.backward(dy)
    yb.backward(dy)
    head_b = rel(rt.segmentation_head[0].bias.grad, ref.segmentation_head[0].bias.grad)
    cos = float(F.cosine_similarity(_flat_grads(rt.named_parameters()), _flat_grads(ref.named_parameters()), dim=0))
    print(f"\n{name} {hw} bf16 storage alone: out {rel(yb, ya):.3e} head-bias grad {head_b:.3e} cosine {cos:.4f}")
    assert 1e-4 < rel(yb, ya) < 1.0


def test_autopad_bf16(gpu_device):
    """40 x 72 pads to 64 x 96 (12 rows / columns on every side) and the output is cropped back"""
    dev = gpu_device
    m, ref = _pair(dev, 11, 4, torch.bfloat16, autopad=True)
    assert m.padding_for(40, 72) == (12, 12, 12, 12)
    x = torch.randn(2, 40, 72, 11, device=dev, generator=gen(dev, 3))
    y, yr = m(x), ref(x.double())
    assert y.shape == yr.shape == (2, 40, 72, 4)
    print(f"\nautopad bf16 out {rel(y, yr):.3e}")
    assert rel(y, yr) <= BF16_OUT, rel(y, yr)
    from py4cast_amd._lib import P4CError

    m2, _ = _pair(dev, 11, 4, torch.bfloat16, autopad=False)
    with pytest.raises(P4CError, match="multiple of 32"):
        m2(x)


def test_native_route_bf16_step(gpu_device):
    from torch.profiler import ProfilerActivity, profile

    from py4cast_amd.customunet import CustomUNetMI355X, CustomUNetSettings

    dev = gpu_device
    torch.manual_seed(0)
    m = CustomUNetMI355X(69, 60, (128, 128), CustomUNetSettings(compute_dtype="bf16", activation_dtype="bf16", encoder_weights=False)).to(dev)
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
                "upsample_nearest", "adaptive_avg_pool", "batch_norm", "dropout"):
        hits = [n for n in low if bad in n and not n.startswith("p4c")]
        assert not hits, (bad, hits[:5])
    assert not [n for n in names if n in ("aten::cat", "aten::convolution", "aten::mm", "aten::addmm", "aten::bmm", "aten::matmul",
                                           "aten::cudnn_convolution", "aten::miopen_convolution", "aten::im2col", "aten::col2im",
                                           "aten::max_pool2d", "aten::max_pool2d_with_indices", "aten::upsample_bilinear2d",
                                           "aten::upsample_nearest2d", "aten::upsample_nearest2d_backward",
                                           "aten::_adaptive_avg_pool2d", "aten::native_batch_norm", "aten::native_dropout")]
    # no concatenation to take apart in the backward: the one slice adjoint of a step is the head's crop from 64 to 60 channels
    assert names.count("aten::slice_backward") == 1
    kernels = " ".join(low)
    assert "up2cat_fwd_kernel" in kernels and "up2cat_bwd_kernel" in kernels and "stem::tail_fwd_kernel<true>" in kernels
    l2, y2, g2 = step(5)
    assert torch.equal(l1, l2) and torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def _lm(dev, key, T=2, H=64, W=64, seed=72, name="resnet18"):
    from helpers import make_dataset_info, synthetic_case
    from py4cast_amd.lightning import AutoRegressiveLightning

    case = synthetic_case(seed=71, B=2, T=T, H=H, W=W, F=12, Ff=5, Fs=4, border=0)
    info = make_dataset_info(case, 5)
    torch.manual_seed(seed)
    lm = AutoRegressiveLightning({"compute_dtype": key, "activation_dtype": key, "encoder_weights": False, "encoder_name": name,
                                  "autopad_enabled": True},
                                 info, None, num_input_steps=1, num_pred_steps_train=T, batch_size=2, model_name="CustomUNet",
                                 losses=[{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}],
                                 training_strategy="diff_ar").to(dev).train()
    return lm, case


def test_graph_replay_equals_eager_step(gpu_device):
    """trainer.GraphedTrainingStep on the bf16 route (one stream, no parallel branches): the replay's loss and gradients are
    bit-identical to the eager step's -- the forward and backward hold no host synchronisation and no data-dependent allocation"""
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


@pytest.mark.parametrize("key", ["f32", "bf16"])
def test_diff_ar_rollout_through_lightning(gpu_device, key):
    """``AutoRegressiveLightning(model_name="CustomUNet")``: 2-step diff_ar rollout at B = 2, 64 x 64, F = 12, Ff = 5, Fs = 4; loss and
    parameter gradients against the float64 restatement driven through the oracle rollout (the float64 statement of the same Lightning
    step).  bf16: the rows come straight from build_x (bf16, zero-padded to the GEMM's 8-channel granularity).  Bars as
    tests/test_deeplabv3_gpu.py::test_scaled_ar_rollout_through_lightning."""
    from helpers import make_batch
    from oracle import losses as olosses
    from oracle import rollout as orollout

    dev = gpu_device
    T = 2
    lm, case = _lm(dev, key, T=T)
    m = lm.model
    assert m.in_channels == 21 and m.out_channels == 12
    seen = []
    hook = m.register_forward_pre_hook(lambda mod, args: seen.append((args[0].dtype, args[0].shape[-1])))
    loss = lm.training_step(make_batch(case, dev), 0)
    loss.backward()
    hook.remove()
    if key == "bf16":
        assert m.rollout_input_format == (torch.bfloat16, 24)
        assert seen == [m.rollout_input_format] * T
    ref = CustomUNetReference(m.in_channels, m.out_channels, "resnet18").double()
    ref.load_state_dict({k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in m.state_dict().items()})
    # the model's training step moved its running statistics T times; the restatement's forward uses batch statistics (train mode)
    ref.train()
    c = {k: (v.double() if v.is_floating_point() else v) for k, v in case.items()}
    statics = c["statics"].unsqueeze(0).expand(2, *c["statics"].shape)
    interior = 1.0 - c["border_mask"]
    pred = orollout.rollout(ref, c["inputs"], c["forcing"], c["outputs"], statics, c["border_mask"], interior, c["diff_std"],
                            c["diff_mean"], training_strategy="diff_ar")
    wts = olosses.weighted_loss_weights(c["state_weight"], c["diff_std"], "mse")
    lref = olosses.weighted_loss(pred, c["outputs"], torch.ones_like(pred), wts, interior, "mse").mean()
    lref.backward()
    rg = dict(ref.named_parameters())
    lerr = abs(loss.item() - lref.item()) / abs(lref.item())
    flat = torch.cat([p.grad.double().flatten().cpu() for p in m.parameters()])
    flat_r = torch.cat([rg[n].grad.flatten() for n, _ in m.named_parameters()])
    cos = float(F.cosine_similarity(flat, flat_r, dim=0))
    print(f"\n{key}: loss {lerr:.3e} cosine {cos:.4f}")
    if key == "f32":
        assert lerr < 2e-4
        worst = max((rel(p.grad.cpu(), rg[n].grad), n) for n, p in m.named_parameters())
        print(f"worst parameter gradient {worst}")
        assert worst[0] < 1e-1, worst
    else:
        assert lerr < 2e-2
        assert cos >= 0.5
