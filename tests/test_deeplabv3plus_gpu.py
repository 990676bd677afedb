"""
DeepLabV3+ (py4cast_amd/deeplabv3plus.py) on the GPU: the multi-rate dilated depthwise 3x3 and the bilinear x4 + concatenation pass
(csrc/deeplabplus.hip) against float64 torch on the same bf16-rounded operands; the whole network against the restatement
(tests/deeplabv3plus_reference.py) in both flavours; the native route of a bf16 step (no library convolution / GEMM / cat / interpolate /
pooling / norm; bit-identical reruns), HIP-graph replay against the eager step and a diff_ar rollout through the Lightning module.

Bars.  Kernels: the project's ``close_bf16`` (<= 6e-3 of the largest magnitude per element, <= 3e-3 in the 2-norm: one bf16 rounding of an
fp32 result is 2^-9 of the element) for every stored map and data gradient, 5e-4 in the 2-norm for the fp32 weight gradients
(tests/test_segformer_gpu.py::test_depthwise_against_float64); moved values (the skip channels, dskip) bit-exact.  fp32 network: output
5e-4, gradients 1e-1 (ReLU / max-pool decisions near a boundary flip between precisions).  bf16 network: RELATIVE to what bf16 storage
alone costs on the same inputs -- the float64 restatement with every stored activation round-tripped through bf16 against the plain one,
no kernel of this package -- output <= 1.5 x that figure, cosine over all parameter gradients >= that cosine - 0.15, head-bias gradient
<= 5e-2 (margins from CustomUNet's record: its native route measured 1.1 x and -0.06 against storage alone).  DeepLabV3's absolute
1.5e-1 / 0.4 are not reachable here: bf16 storage alone misses them with resnet34.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import step_reference as R  # noqa: E402
from deeplabv3plus_reference import DeepLabV3PlusReference, bf16_round_trip  # noqa: E402

pytestmark = pytest.mark.gpu

GRID_CAP_OCTETS = 2048 * 256      # csrc/deeplabplus.hip: at most 2048 workgroups of 256 threads, one octet per thread and trip


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


# ------------------------------------------------------------------------------------------------ depthwise 3x3, R rates
DW_CASES = [(1, 1, 1, 8, (12, 24, 36)),          # every non-centre tap is outside
            (2, 40, 28, 24, (12, 24, 36)),       # non-square: rate 36 lands inside along H only, rate 24 along both; C no multiple of 16
            (2, 14, 13, 512, (12, 24, 36)),      # the stride-16 map of a 224 x 208 input
            (2, 32, 32, 512, (12, 24, 36)),      # the bench map (512 x 512)
            (2, 128, 128, 304, (1,)),            # block2 at 512 x 512: past one trip of the grid-stride loop
            (2, 9, 7, 8, (1, 2)),                # R = 2, small dilations
            (1, 5, 6, 520, (1, 2))]              # 65 octets: dw_wgrad's second channel block (gridDim.y = 2), one active lane in it


def _dw_operands(dev, B, H, W, C, rates):
    g = gen(dev, H * W + C + len(rates))
    x = torch.randn(B, H, W, C, device=dev, generator=g).to(torch.bfloat16)
    ws = [(0.3 * torch.randn(C, 1, 3, 3, device=dev, generator=g)) for _ in rates]
    dys = [torch.randn(B, H, W, C, device=dev, generator=g).to(torch.bfloat16) for _ in rates]
    return x, ws, dys


@pytest.mark.parametrize("B,H,W,C,rates", DW_CASES)
def test_depthwise_dilated_against_float64(gpu_device, B, H, W, C, rates):
    """y_r, dx = sum_r (one launch each) and every dw_r against float64 F.conv2d(groups=C, padding=d, dilation=d) and its autograd on the
    same operands.  Launch geometry (csrc/deeplabplus.hip): a thread owns one 8-channel octet of one pixel, 256 threads per workgroup,
    GRID_CAP = 2048 workgroups -- one trip of the grid-stride loop covers 524288 octets.  (2, 128, 128, 304, (1,)) has
    2 * 128 * 128 * 38 = 1245184 octets: the loop takes a second and a third trip."""
    from py4cast_amd.deeplabv3plus import depthwise3x3_dilated

    dev = gpu_device
    if (H, C) == (128, 304):
        assert B * H * W * (C // 8) == 1245184 > GRID_CAP_OCTETS
    if C == 520:    # the weight gradient's grid is (pixel chunks, ceil(octets / 64), R): every other case and every network has C <= 512
        assert (C // 8 + 63) // 64 == 2 and C // 8 - 64 == 1
    x, ws, dys = _dw_operands(dev, B, H, W, C, rates)
    xg = x.clone().requires_grad_(True)
    wg = [w.clone().requires_grad_(True) for w in ws]
    ys = depthwise3x3_dilated(xg, wg, rates)
    assert len(ys) == len(rates)
    torch.autograd.backward(list(ys), dys)
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = [w.double().requires_grad_(True) for w in ws]
    refs = [F.conv2d(x64, w, padding=d, dilation=d, groups=C) for w, d in zip(w64, rates)]
    torch.autograd.backward(refs, [dy.double().permute(0, 3, 1, 2) for dy in dys])
    for r, (y, ref) in enumerate(zip(ys, refs)):
        assert y.dtype == torch.bfloat16 and y.shape == (B, H, W, C)
        close_bf16(y.float().permute(0, 3, 1, 2), ref, f"y_{r} (rate {rates[r]})")
    close_bf16(xg.grad.float().permute(0, 3, 1, 2), x64.grad, "dx")
    for r, (w, wr) in enumerate(zip(wg, w64)):
        assert w.grad.shape == (C, 1, 3, 3) and w.grad.dtype == torch.float32
        assert rel(w.grad, wr.grad) <= 5e-4, (r, rates[r], rel(w.grad, wr.grad))
    if H == 1:      # a 1 x 1 map: only the centre taps see data
        for w in wg:
            off = w.grad.reshape(C, 9)[:, [0, 1, 2, 3, 5, 6, 7, 8]]
            assert bool((off == 0).all())


@pytest.mark.parametrize("B,H,W,C,rates", [DW_CASES[1], DW_CASES[3]])
def test_depthwise_dilated_rerun_is_bit_identical(gpu_device, B, H, W, C, rates):
    from py4cast_amd.deeplabv3plus import depthwise3x3_dilated

    x, ws, dys = _dw_operands(gpu_device, B, H, W, C, rates)

    def run():
        xg = x.clone().requires_grad_(True)
        wg = [w.clone().requires_grad_(True) for w in ws]
        ys = depthwise3x3_dilated(xg, wg, rates)
        torch.autograd.backward(list(ys), dys)
        return [y.detach() for y in ys] + [xg.grad] + [w.grad for w in wg]

    a, b = run(), run()
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_depthwise_one_launch_equals_single_rate_launches(gpu_device):
    """the three-rate launch's maps are those of three single-rate launches of the same kernel, bit for bit (same taps, same order)"""
    from py4cast_amd.deeplabv3plus import depthwise3x3_dilated

    x, ws, _ = _dw_operands(gpu_device, 2, 40, 28, 24, (12, 24, 36))
    ys = depthwise3x3_dilated(x, ws, (12, 24, 36))
    for y, w, d in zip(ys, ws, (12, 24, 36)):
        assert torch.equal(y, depthwise3x3_dilated(x, [w], (d,))[0])


def test_depthwise_dilated_rejects_what_it_does_not_serve(gpu_device):
    from py4cast_amd._lib import P4CError
    from py4cast_amd.deeplabv3plus import depthwise3x3_dilated

    dev = gpu_device
    x = torch.zeros(1, 4, 4, 16, device=dev, dtype=torch.bfloat16)
    w = torch.zeros(16, 1, 3, 3, device=dev)
    with pytest.raises(P4CError):
        depthwise3x3_dilated(x[..., :12].contiguous(), [w[:12]], (1,))       # C = 12: off the 8-channel granularity
    with pytest.raises(P4CError):
        depthwise3x3_dilated(x, [w] * 4, (1, 2, 3, 4))                       # R = 4
    with pytest.raises(P4CError):
        depthwise3x3_dilated(x, [w], (0,))                                   # rate 0
    with pytest.raises(P4CError):
        depthwise3x3_dilated(x.float(), [w], (1,))                           # fp32 x
    with pytest.raises(P4CError):
        depthwise3x3_dilated(x, [w, w], (1,))                                # rates and weights of different lengths
    assert depthwise3x3_dilated(x, [w], (1,))[0].shape == x.shape


# ------------------------------------------------------------------------------------------------ bilinear x4 + concatenation
@pytest.mark.parametrize("B,h,w,Ca,Cs,ld", [(1, 1, 1, 8, 8, None),            # in_size 1: ac_scale = 0
                                            (2, 3, 5, 8, 16, None),           # small, non-square
                                            (2, 8, 6, 256, 48, None),         # the 128 x 96 network's decoder, ld = 304
                                            (2, 32, 32, 256, 48, None),       # the bench decoder: past one loop trip
                                            (2, 5, 7, 16, 8, 40)])            # ld > Ca + Cs: the pad channels come out as zeros
def test_up_cat_against_float64(gpu_device, B, h, w, Ca, Cs, ld):
    """out = [bilinear_align_corners_x4(a) | skip | zeros] against torch.cat([F.interpolate(a, scale_factor=4, mode="bilinear",
    align_corners=True), skip]) in float64.  The skip channels and dskip are moved values: bit-exact; the up-sampled channels and da pass
    close_bf16 and equal upsample_bilinear_ac(a, 4) bit for bit (one statement of the arithmetic: csrc/resize_ac.hpp).  The wrapper
    promises ZEROS in the channels from Ca + Cs on.  Launch geometry: one octet of one output pixel's ld-wide row per thread, 2048
    workgroups of 256 at most -- 524288 octets per trip; (2, 32, 32, 256, 48) writes 2 * 128 * 128 * 38 = 1245184: three trips; its
    backward has 2 * 32 * 32 * 32 + 2 * 128 * 128 * 6 = 262144 units."""
    from py4cast_amd.deeplabv3 import upsample_bilinear_ac
    from py4cast_amd.deeplabv3plus import up_cat

    dev = gpu_device
    s = 4
    width = Ca + Cs if ld is None else ld
    if (h, Ca) == (32, 256):
        assert B * s * h * s * w * (width // 8) == 1245184 > GRID_CAP_OCTETS
    g = gen(dev, h * w + Ca)
    a = torch.randn(B, h, w, Ca, device=dev, generator=g).to(torch.bfloat16)
    skip = torch.randn(B, s * h, s * w, Cs, device=dev, generator=g).to(torch.bfloat16)
    ag, sg = a.clone().requires_grad_(True), skip.clone().requires_grad_(True)
    out = up_cat(ag, sg, s) if ld is None else up_cat(ag, sg, s, ld=ld)
    assert out.shape == (B, s * h, s * w, width) and out.dtype == torch.bfloat16
    a64 = a.double().permute(0, 3, 1, 2).requires_grad_(True)
    up64 = F.interpolate(a64, scale_factor=s, mode="bilinear", align_corners=True)
    assert torch.equal(out.detach()[..., Ca: Ca + Cs], skip)
    close_bf16(out.detach()[..., :Ca].float().permute(0, 3, 1, 2), up64, "up-sampled channels")
    assert torch.equal(out.detach()[..., :Ca], upsample_bilinear_ac(a, s))
    if width > Ca + Cs:
        assert bool((out.detach()[..., Ca + Cs:] == 0).all())
    dout = torch.randn(out.shape, device=dev, generator=g).to(torch.bfloat16)
    out.backward(dout)
    assert torch.equal(sg.grad, dout[..., Ca: Ca + Cs])
    up64.backward(dout[..., :Ca].double().permute(0, 3, 1, 2))
    close_bf16(ag.grad.float().permute(0, 3, 1, 2), a64.grad, "da")
    # the same adjoint as the stand-alone up-sampling's, bit for bit
    a2 = a.clone().requires_grad_(True)
    upsample_bilinear_ac(a2, s).backward(dout[..., :Ca].contiguous())
    assert torch.equal(ag.grad, a2.grad)


def test_up_cat_rejects_what_it_does_not_serve(gpu_device):
    from py4cast_amd._lib import P4CError
    from py4cast_amd.deeplabv3plus import up_cat

    dev = gpu_device
    a = torch.zeros(1, 2, 2, 8, device=dev, dtype=torch.bfloat16)
    skip = torch.zeros(1, 8, 8, 8, device=dev, dtype=torch.bfloat16)
    for call in (lambda: up_cat(a[..., :4], skip, 4),                       # Ca off the 8-channel granularity
                 lambda: up_cat(a, skip[:, :7], 4),                         # not the x4 grid
                 lambda: up_cat(a.float(), skip, 4),
                 lambda: up_cat(a, skip, 9),                                # scale beyond 8
                 lambda: up_cat(a, skip, 4, ld=12),                         # ld < Ca + Cs
                 lambda: up_cat(a, skip, 4, ld=20)):                        # ld off the 8-channel granularity
        with pytest.raises(P4CError):
            call()
    assert up_cat(a, skip, 4).shape == (1, 8, 8, 16)


# ------------------------------------------------------------------------------------------------ the network
FP32_OUT = 5e-4
FP32_GRAD = 1e-1
BF16_OUT_FACTOR = 1.5       # x the storage-alone output error
BF16_COS_MARGIN = 0.15      # below the storage-alone cosine
BF16_HEAD = 5e-2
NET_CASES = [("resnet18", (128, 96)), ("resnet18", (224, 208)), ("resnet34", (128, 96))]
CIN, COUT = 69, 60


def _model(dev, dtype, name, seed=0, dc=256):
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    key = "bf16" if dtype == torch.bfloat16 else "f32"
    torch.manual_seed(seed)
    return DeepLabV3PlusMI355X(CIN, COUT, None, DeepLabV3PlusSettings(encoder_name=name, encoder_weights=False, decoder_channels=dc, aspp_dropout=0.0,
                                                                      compute_dtype=key, activation_dtype=key)).to(dev).train()


def _flat_grads(named):
    return torch.cat([p.grad.double().flatten() for _, p in named])


def _distinct_samples(x):
    """the two samples of a batch at different levels and amplitudes (sample 1 = 2 x + 0.5), as fields of different dates are.  Why: the
    ASPP pooling branch normalises ONE value per (sample, channel) over the batch; at B = 2 that is delta / sqrt(delta^2 + eps) with
    delta = half the difference of the two samples' pooled features, and its derivative eps / (delta^2 + eps)^1.5 is negligible for
    |delta| >> sqrt(eps) but reaches 1 / sqrt(eps) = 316 at delta = 0.  Two i.i.d. N(0, 1) samples have nearly equal pooled features: a
    few channels then sit at delta ~ 0, their gradient floods the encoder (the pooled gradient is broadcast to every pixel) and the
    cosine over all parameter gradients becomes the cosine of those few ill-conditioned numbers -- in float64 on the CPU, with no kernel
    of this package, bf16 storage alone then scatters between 0.43 and 0.70 from one draw to the next, and rounding the GEMM weights to
    bf16 as well moves it by +-0.17: no route could be held to a 0.15 margin there.  With distinct samples the same measurement gives
    0.69 ... 0.90 for storage alone and 0.84 ... 0.86 with rounded weights."""
    x = x.clone()
    x[1] = 2 * x[1] + 0.5
    return x


_REFERENCE = {}


def _reference(dev, name, hw, state):
    """the float64 restatement's results on the case's weights and inputs, computed once per (encoder, grid) and shared by both flavours:
    train output, gradients, running statistics, eval output -- and the same from the restatement with every stored activation
    round-tripped through bf16 (what bf16 storage alone costs: no kernel of this package runs)"""
    if (name, hw) in _REFERENCE:
        return _REFERENCE[(name, hw)]
    g = gen(dev, 7)
    x = _distinct_samples(torch.randn(2, *hw, CIN, device=dev, generator=g))
    dy = torch.randn(2, *hw, COUT, device=dev, generator=g)
    res = {"x": x, "dy": dy}
    for tag, rt in (("plain", None), ("storage", bf16_round_trip)):
        ref = DeepLabV3PlusReference(CIN, COUT, name, round_trip=rt).to(dev).double().train()
        ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in state.items()})
        xd = x.double().requires_grad_(True)
        y = ref(xd)
        y.backward(dy.double())
        res[tag] = {"y": y.detach(), "dx": xd.grad, "grads": {n: p.grad for n, p in ref.named_parameters()},
                    "buffers": {n: b.detach().clone() for n, b in ref.named_buffers()}}
        ref.eval()
        with torch.no_grad():
            res[tag]["y_eval"] = ref(x.double())
    names = list(res["plain"]["grads"])
    flat = {t: torch.cat([res[t]["grads"][n].flatten() for n in names]) for t in ("plain", "storage")}
    res["storage_out"] = rel(res["storage"]["y"], res["plain"]["y"])
    res["storage_eval"] = rel(res["storage"]["y_eval"], res["plain"]["y_eval"])
    res["storage_cos"] = float(F.cosine_similarity(flat["storage"], flat["plain"], dim=0))
    res["storage_head"] = rel(res["storage"]["grads"]["segmentation_head.0.bias"], res["plain"]["grads"]["segmentation_head.0.bias"])
    _REFERENCE[(name, hw)] = res
    return res


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name,hw", NET_CASES)
def test_network_against_restatement(gpu_device, dtype, name, hw):
    """both flavours against the float64 restatement on the same weights and inputs (69 -> 60 channels, dc = 256, aspp_dropout 0),
    training forward + backward, then eval.  2 x 224 x 208: the stride-16 map is 14 x 13, where rate-12 taps land inside the map.
    fp32 (library operations): output 5e-4, gradients 1e-1.
    bf16 (the native route): against what bf16 storage alone costs on the same inputs, measured here (module docstring): output <=
    1.5 x, cosine over all parameter gradients >= storage's - 0.15, head-bias gradient <= 5e-2.
    Measured (resnet18 128 x 96, resnet18 224 x 208, resnet34 128 x 96):
    fp32: output 1.4e-4, 2.3e-5, 4.4e-5; input gradient 3.2e-2, 3.0e-3, 1.2e-2; worst parameter gradient 6.3e-2 (the pooling branch's
    convolution), 3.7e-3, 1.7e-2; eval output 8.3e-6, 1.4e-6, 1.6e-6.
    bf16: output 6.9e-2, 6.4e-2, 1.42e-1 against storage alone 5.1e-2, 6.0e-2, 1.43e-1 (x 1.35, 1.07, 0.99 of 1.5); cosine 0.873, 0.879,
    0.594 against storage alone 0.874, 0.849, 0.682 (-0.001, +0.030, -0.088 of -0.15); head-bias gradient 2.3e-3, 2.4e-3, 2.3e-3 of
    5e-2; eval output 8.0e-3, 7.4e-3, 8.1e-3 against storage alone 5.7e-3, 6.0e-3, 8.1e-3 (x 1.39, 1.24, 0.99).
    The inputs are _distinct_samples (its docstring says why); with two i.i.d. N(0, 1) samples resnet18 at 128 x 96 measured cosine
    0.387 against storage alone 0.695 here -- every decoder parameter within 0.02 of its storage-alone cosine, the whole gap in the
    encoder and the pooling branch's convolution, i.e. behind that branch's batch norm over two values."""
    dev = gpu_device
    m = _model(dev, dtype, name)
    ref = _reference(dev, name, hw, m.state_dict())
    plain = ref["plain"]
    x = ref["x"]
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    assert y.shape == plain["y"].shape == (2, *hw, COUT)
    y.float().backward(ref["dy"])
    out = rel(y, plain["y"])
    head_b = rel(m.segmentation_head[0].bias.grad, plain["grads"]["segmentation_head.0.bias"])
    flat_r = torch.cat([plain["grads"][n].flatten() for n, _ in m.named_parameters()])
    cos = float(F.cosine_similarity(_flat_grads(m.named_parameters()), flat_r, dim=0))
    print(f"\n{name} {hw} {dtype}: out {out:.3e} head-bias grad {head_b:.3e} cosine {cos:.4f} dx {rel(xg.grad, plain['dx']):.3e} | bf16 storage "
          f"alone: out {ref['storage_out']:.3e} head-bias grad {ref['storage_head']:.3e} cosine {ref['storage_cos']:.4f} eval "
          f"{ref['storage_eval']:.3e}")
    assert 1e-4 < ref["storage_out"] < 1.0      # the storage-alone figure is what bf16 predicts: above fp32's, below O(1)
    if dtype == torch.float32:
        assert out <= FP32_OUT, out
        assert rel(xg.grad, plain["dx"]) <= FP32_GRAD, rel(xg.grad, plain["dx"])
        worst = max((rel(p.grad, plain["grads"][n]), n) for n, p in m.named_parameters())
        print(f"worst parameter gradient {worst}")
        assert worst[0] <= FP32_GRAD, worst
    else:
        assert out <= BF16_OUT_FACTOR * ref["storage_out"], (out, ref["storage_out"])
        assert cos >= ref["storage_cos"] - BF16_COS_MARGIN, (cos, ref["storage_cos"])
        assert head_b <= BF16_HEAD, head_b
    for n, b in m.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            bar = 2 * FP32_OUT if dtype == torch.float32 else BF16_OUT_FACTOR * max(ref["storage_out"], rel(ref["storage"]["buffers"][n], plain["buffers"][n]))
            assert rel(b, plain["buffers"][n]) <= bar, (n, rel(b, plain["buffers"][n]), bar)
    m.eval()
    with torch.no_grad():
        ye = m(x)
    print(f"eval out {rel(ye, plain['y_eval']):.3e}")
    assert rel(ye, plain["y_eval"]) <= (FP32_OUT if dtype == torch.float32 else BF16_OUT_FACTOR * ref["storage_eval"]), rel(ye, plain["y_eval"])


def test_grid_and_batch_checks(gpu_device):
    dev = gpu_device
    m = _model(dev, torch.bfloat16, "resnet18", dc=32)
    with pytest.raises(RuntimeError, match="divisible by 16"):
        m(torch.randn(2, 72, 64, CIN, device=dev))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(torch.randn(1, 64, 64, CIN, device=dev))
    m.eval()
    with torch.no_grad():
        assert m(torch.randn(1, 64, 48, CIN, device=dev)).shape == (1, 64, 48, COUT)


def test_native_route_bf16_step(gpu_device, monkeypatch):
    """a profiled bf16 training step at 2 x 128 x 128, 69 -> 60 (the default Dropout(0.5) included): no library convolution / GEMM / cat /
    interpolate / pooling / norm / dropout kernel; the three ASPP rates from ONE depthwise launch each way (3 depthwise launches per
    direction: the ASPP's, aspp.1's and block2's); one up_cat each way; reruns from the same seed bit-identical"""
    from torch.profiler import ProfilerActivity, profile

    from py4cast_amd import _lib as L
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    dev = gpu_device
    torch.manual_seed(0)
    m = DeepLabV3PlusMI355X(69, 60, (128, 128), DeepLabV3PlusSettings(compute_dtype="bf16", activation_dtype="bf16", encoder_weights=False)).to(dev)
    x = torch.randn(2, 128, 128, 72, device=dev).to(torch.bfloat16)
    x[..., 69:] = 0
    calls = []
    real_call = L.call

    def counting_call(name, *a, **k):
        calls.append((name, a))
        return real_call(name, *a, **k)

    monkeypatch.setattr(L, "call", counting_call)

    def step(seed):
        torch.manual_seed(seed)
        m.zero_grad(set_to_none=True)
        y = m(x)
        loss = y.float().square().mean()
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), y.detach().clone(), [p.grad.detach().clone() for p in m.parameters()]

    step(5)
    calls.clear()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        l1, y1, g1 = step(5)
    assert m.last_dropout_mask is not None and m.last_dropout_mask.shape == (2 * 8 * 8, 256)
    names = [e.name for e in prof.events()]
    low = [n.lower() for n in names]
    for bad in ("miopen", "cudnn", "hipblaslt", "rocblas", "cijk_", "im2col", "col2im", "catarray", "max_pool", "upsample_bilinear",
                "upsample_nearest", "adaptive_avg_pool", "batch_norm", "dropout", "conv_depthwise"):
        hits = [n for n in low if bad in n and not n.startswith("p4c")]
        assert not hits, (bad, hits[:5])
    assert not [n for n in names if n in ("aten::cat", "aten::convolution", "aten::mm", "aten::addmm", "aten::bmm", "aten::matmul",
                                           "aten::cudnn_convolution", "aten::miopen_convolution", "aten::_conv_depthwise2d", "aten::im2col",
                                           "aten::col2im", "aten::max_pool2d", "aten::max_pool2d_with_indices", "aten::upsample_bilinear2d",
                                           "aten::upsample_bilinear2d_backward", "aten::_adaptive_avg_pool2d", "aten::native_batch_norm",
                                           "aten::native_dropout")]
    count = {n: sum(1 for c, _ in calls if c == n) for n in {c for c, _ in calls}}
    assert count["p4c_dlp_dw3x3_fwd"] == 3 and count["p4c_dlp_dw3x3_dgrad"] == 3 and count["p4c_dlp_dw3x3_wgrad"] == 3, count
    assert count["p4c_dlp_up_cat_fwd"] == 1 and count["p4c_dlp_up_cat_bwd"] == 1, count
    assert count["p4c_upsample_bilinear_ac_fwd"] == 1 and count["p4c_upsample_bilinear_ac_bwd"] == 1, count      # the head's alone
    kernels = " ".join(low)
    for k in ("dw_fwd_kernel<3>", "dw_fwd_kernel<1>", "dw_dgrad_kernel<3>", "dw_dgrad_kernel<1>", "dw_wgrad_kernel", "upcat_fwd_kernel",
              "upcat_bwd_kernel"):
        assert k in kernels, k
    l2, y2, g2 = step(5)
    assert torch.equal(l1, l2) and torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


# ------------------------------------------------------------------------------------------------ through the Lightning module
LM_T, LM_H, LM_W = 2, 128, 96


def _lm(dev, key, dropout=0.0, seed=72):
    from helpers import make_dataset_info, synthetic_case
    from py4cast_amd.lightning import AutoRegressiveLightning

    case = synthetic_case(seed=71, B=2, T=LM_T, H=LM_H, W=LM_W, F=12, Ff=5, Fs=4, border=0)
    case["inputs"] = _distinct_samples(case["inputs"])      # (the pooling branch's batch norm over B = 2: see _distinct_samples)
    info = make_dataset_info(case, 5)
    torch.manual_seed(seed)
    lm = AutoRegressiveLightning({"compute_dtype": key, "activation_dtype": key, "encoder_weights": False, "aspp_dropout": dropout, "upsampling": 8},
                                 info, None, num_input_steps=1, num_pred_steps_train=LM_T, batch_size=2, model_name="DeepLabV3Plus",
                                 losses=[{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}],
                                 training_strategy="diff_ar").to(dev).train()
    return lm, case


@pytest.mark.parametrize("dropout", [0.0, 0.5])
def test_graph_replay_equals_eager_step(gpu_device, dropout):
    """trainer.GraphedTrainingStep on the bf16 route (one stream, no parallel branches): with the generator at the same state, the
    replay's loss and gradients are bit-identical to the eager step's (the Dropout draws included) -- the forward and backward hold no
    host synchronisation and no data-dependent allocation"""
    from helpers import make_batch
    from py4cast_amd.trainer import FlatDDP, GraphedTrainingStep

    dev = gpu_device
    lm, case = _lm(dev, "bf16", dropout=dropout)
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


def _reference_rollout(ref, c, dev):
    """the 2-step diff_ar rollout and its weighted MSE in float64, from the element references of tests/step_reference.py (graph layout:
    grid points flat): x = build_x(state, statics, forcing_t); state = state + net(x) (diff_ar: no scaling, no border forcing); loss =
    mean over (b, t) of the weighted loss.  Returns (loss, prediction (B, T, N, F))."""
    B, T, H, W, Fe = c["outputs"].shape
    N = H * W
    flat = lambda t: t.reshape(*t.shape[:-3], N, t.shape[-1])             # noqa: E731
    state = flat(c["inputs"]).double()                                    # (B, 1, N, F)
    statics = flat(c["statics"]).double().unsqueeze(0).expand(B, N, -1)
    preds = []
    for t in range(T):
        x = R.build_x(state, statics, flat(c["forcing"][:, t]).double(), out_dtype=torch.float64)
        y = ref(x.view(B, H, W, -1)).reshape(B, N, Fe)
        new = R.ar_update(state[:, -1], y)
        preds.append(new)
        state = new.unsqueeze(1)
    pred = torch.stack(preds, dim=1)
    interior = (1.0 - flat(c["border_mask"]).double()).reshape(N)
    weights = c["state_weight"].double() / c["diff_std"].double() ** 2   # losses.py:110-124, MSE
    loss = R.weighted_loss(pred, flat(c["outputs"]).double(), weights, interior, "mse").mean()
    return loss, pred, weights


@pytest.mark.parametrize("key", ["f32", "bf16"])
def test_diff_ar_rollout_through_lightning(gpu_device, key):
    """``AutoRegressiveLightning(model_name="DeepLabV3Plus")`` built from the yaml's ``upsampling: 8``: 2-step diff_ar rollout at B = 2,
    128 x 96, F = 12, Ff = 5, Fs = 4; loss and parameter gradients against the float64 restatement driven through the rollout and loss of
    tests/step_reference.py; then a predict_step of the right shape.  bf16: the rows come straight from build_x (bf16, zero-padded to the
    GEMM's 8-channel granularity).
    Bars.  fp32: loss 1e-3 -- the loss is quadratic in (prediction - target), and an output error of 5e-4 (FP32_OUT) of a prediction
    whose residual against the N(0, 1) targets is at least as large as the output moves it by at most (1 + 5e-4)^2 - 1; parameter
    gradients 1e-1.  bf16: against the same rollout with the storage-alone restatement: with delta = the weighted 2-norm of its
    prediction error over the weighted 2-norm of the plain residual, sqrt(L) moves by at most delta, so the loss by (1 + delta)^2 - 1; the
    native route gets the bound of 1.5 x delta (BF16_OUT_FACTOR); cosine over all parameter gradients >= storage's - 0.15.
    Measured: fp32 loss 4.0e-6, worst parameter gradient 2.9e-2 (cosine 0.9997); bf16 loss 8.0e-3 of 1.6e-1 (storage alone 4.2e-3,
    delta 5.1e-2), cosine 0.435 against storage alone 0.424."""
    from helpers import make_batch

    dev = gpu_device
    lm, case = _lm(dev, key)
    m = lm.model
    assert m.in_channels == 21 and m.out_channels == 12 and m.settings.upsampling == 8
    seen = []
    hook = m.register_forward_pre_hook(lambda mod, args: seen.append((args[0].dtype, args[0].shape[-1])))
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    loss = lm.training_step(make_batch(case, dev), 0)
    loss.backward()
    hook.remove()
    if key == "bf16":
        assert m.rollout_input_format == (torch.bfloat16, 24)
        assert seen == [m.rollout_input_format] * LM_T
    c = {k: v.to(dev) for k, v in case.items()}
    out = {}
    for tag, rt in (("plain", None),) + ((("storage", bf16_round_trip),) if key == "bf16" else ()):
        ref = DeepLabV3PlusReference(m.in_channels, m.out_channels, "resnet18", round_trip=rt).to(dev).double().train()
        ref.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in state0.items()})
        lref, pred, weights = _reference_rollout(ref, c, dev)
        lref.backward()
        out[tag] = (lref.detach(), pred.detach(), {n: p.grad for n, p in ref.named_parameters()})
    lref, pred, rg = out["plain"]
    lerr = abs(loss.item() - lref.item()) / abs(lref.item())
    flat = torch.cat([p.grad.double().flatten() for p in m.parameters()])
    flat_r = torch.cat([rg[n].flatten() for n, _ in m.named_parameters()])
    cos = float(F.cosine_similarity(flat, flat_r, dim=0))
    print(f"\n{key}: loss {lerr:.3e} cosine {cos:.4f}")
    if key == "f32":
        assert lerr <= 1e-3, lerr
        worst = max((rel(p.grad, rg[n]), n) for n, p in m.named_parameters())
        print(f"worst parameter gradient {worst}")
        assert worst[0] <= FP32_GRAD, worst
    else:
        ls, ps, sg = out["storage"]
        tgt = c["outputs"].double().reshape(pred.shape)
        delta = float((((ps - pred) ** 2 * weights).sum() / ((pred - tgt) ** 2 * weights).sum()).sqrt())
        cos_s = float(F.cosine_similarity(torch.cat([sg[n].flatten() for n, _ in m.named_parameters()]), flat_r, dim=0))
        bar = (1 + BF16_OUT_FACTOR * delta) ** 2 - 1
        print(f"bf16 storage alone: loss {abs(ls.item() - lref.item()) / abs(lref.item()):.3e} delta {delta:.3e} cosine {cos_s:.4f}; loss bar {bar:.3e}")
        assert lerr <= bar, (lerr, bar)
        assert cos >= cos_s - BF16_COS_MARGIN, (cos, cos_s)
    lm.eval()
    with torch.no_grad():
        preds = lm.predict_step(make_batch(case, dev), 0)
    assert preds.tensor.shape == (2, LM_T, LM_H, LM_W, 12) and bool(torch.isfinite(preds.tensor.float()).all())
