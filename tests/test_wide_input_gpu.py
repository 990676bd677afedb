"""
HalfUNet fed num_input_steps >= 2 past states (in_channels = T_in * F + Fs + Ff up to 256): the K-chunked first convolution
(conv_fwd_f32_wide / conv_fwd_bf16_wide), its weight gradient over 64-channel chunks and its data gradient over several
64-channel output blocks, through the C ABI; the whole plan against the oracle with the gradient of EVERY input channel; and the
rollout with two input states against the float64 oracle.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _bf(t):
    return t.bfloat16().double()


def _noise_bar(err32, floor):
    # as tests/test_model_gpu.py: the larger of a floor and 10x torch's own fp32 CPU error against the float64 oracle
    return max(floor, 10.0 * err32)


def _operands(CI, CIreal, H, W, seed, B=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, CI, generator=g)
    x[..., CIreal:] = 0
    w = torch.randn(64, CIreal, 3, 3, generator=g) * 0.05
    scale = torch.rand(B, CI, generator=g) + 0.5
    shift = torch.randn(B, CI, generator=g) * 0.3
    return x, w, scale, shift


WIDE = [(128, 100, 16, 32), (160, 129, 24, 40), (192, 189, 8, 64), (256, 250, 20, 48)]


@pytest.mark.parametrize("CI,CIreal,H,W", WIDE)
def test_wide_conv_fwd_f32_matches_float64(gpu_device, CI, CIreal, H, W):
    from py4cast_amd import ops_model as om

    x, w, scale, shift = _operands(CI, CIreal, H, W, CI + H)
    wp = om.prep_weights(w.to(gpu_device), False, 64, CI)
    for transform in (False, True):
        xin = torch.relu(x * scale[:, None, None, :] + shift[:, None, None, :]) if transform else x
        ref = Fn.conv2d(xin[..., :CIreal].double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
        out, stats = om.conv_fwd(x.to(gpu_device), wp, 3, in_scale=scale.to(gpu_device) if transform else None,
                                 in_shift=shift.to(gpu_device) if transform else None, in_relu=transform, want_stats=True)
        assert rel_err(out, ref) < 1e-4
        s = stats.sum(0).cpu().double()
        np.testing.assert_allclose(s[0].numpy(), ref.sum((0, 1, 2)).numpy(), rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(s[1].numpy(), (ref**2).sum((0, 1, 2)).numpy(), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("storage", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("CI,CIreal,H,W", WIDE + [(160, 129, 64, 64)])
def test_wide_conv_fwd_bf16_matches_rounded_reference(gpu_device, CI, CIreal, H, W, storage):
    from py4cast_amd import ops_model as om

    x, w, scale, shift = _operands(CI, CIreal, H, W, CI + 7 * H)
    x = x.to(storage).float()   # what the kernel reads
    wp = om.prep_weights(w.to(gpu_device), False, 64, CI, compute="bf16")
    for transform in (False, True):
        xin = torch.relu(x * scale[:, None, None, :] + shift[:, None, None, :]) if transform else x
        ref = Fn.conv2d(_bf(xin[..., :CIreal]).permute(0, 3, 1, 2), _bf(w), padding=1).permute(0, 2, 3, 1)
        if storage == torch.bfloat16:
            ref = _bf(ref)   # rounded once, on store
        out, stats = om.conv_fwd(x.to(storage).to(gpu_device), wp, 3, in_scale=scale.to(gpu_device) if transform else None,
                                 in_shift=shift.to(gpu_device) if transform else None, in_relu=transform, want_stats=True,
                                 compute="bf16")
        assert out.dtype == storage
        bar = 5e-4 if transform else 2e-5
        if storage == torch.bfloat16:
            bar = max(bar, 1e-2)   # one bf16 ulp (2^-8 .. 2^-7 relative) where the two fp32 sums round to different sides
        assert rel_err(out, ref) < bar
        # statistics slots: the sums of the stored values
        assert stats.shape[0] == 2 * ((H + 7) // 8) * ((W + 31) // 32)
        s = stats.sum(0).cpu().double()
        stored = out.detach().cpu().double()
        np.testing.assert_allclose(s[0].numpy(), stored.sum((0, 1, 2)).numpy(), rtol=1e-4, atol=1e-2)
        np.testing.assert_allclose(s[1].numpy(), (stored**2).sum((0, 1, 2)).numpy(), rtol=1e-4, atol=1e-2)
        np.testing.assert_allclose(s[0].numpy(), ref.sum((0, 1, 2)).numpy(), rtol=2e-3, atol=5e-2)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("CI,CIreal,H,W", [(160, 129, 16, 64), (256, 250, 8, 32), (192, 189, 12, 40)])
def test_wide_conv_weight_grad_over_chunks(gpu_device, CI, CIreal, H, W, compute):
    from py4cast_amd import ops_model as om

    x, _, scale, shift = _operands(CI, CIreal, H, W, CI + 3 * W)
    g = torch.Generator().manual_seed(CI)
    dout = torch.randn(2, H, W, 64, generator=g)
    if compute == "bf16":
        x, dout = _bf(x).float(), _bf(dout).float()
    w = torch.zeros(64, CIreal, 3, 3, dtype=torch.float64, requires_grad=True)
    xin = x[..., :CIreal].double()
    Fn.conv2d(xin.permute(0, 3, 1, 2), w, padding=1).backward(dout.double().permute(0, 3, 1, 2))
    grad = torch.ones(64, CIreal, 3, 3, device=gpu_device)   # accumulation semantics: += on top of ones
    om.conv_wgrad(x.to(gpu_device), dout.to(gpu_device), 3, 64, CIreal, grad, compute=compute)
    assert rel_err(grad - 1.0, w.grad) < (2e-5 if compute == "f32" else 1e-4)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("CIreal", [120, 129, 189, 256])
def test_wide_conv_data_grad_over_output_blocks(gpu_device, CIreal, compute):
    """dL/dx of the first convolution for 2..4 output blocks of 64 input channels (120: a ragged last block)."""
    from py4cast_amd import ops_model as om

    H, W = 16, 40
    blocks = (CIreal + 63) // 64
    g = torch.Generator().manual_seed(CIreal)
    w = torch.randn(64, CIreal, 3, 3, generator=g) * 0.05
    dout = torch.randn(2, H, W, 64, generator=g)
    if compute == "bf16":
        w, dout = _bf(w).float(), _bf(dout).float()
    x = torch.zeros(2, CIreal, H, W, dtype=torch.float64, requires_grad=True)
    Fn.conv2d(x, w.double(), padding=1).backward(dout.double().permute(0, 3, 1, 2))
    ref = x.grad.permute(0, 2, 3, 1)
    wp = om.prep_weights(w.to(gpu_device), True, 64 * blocks, 64, compute=compute)
    got = om.conv_fwd(dout.to(gpu_device), wp, 3, m_blocks=blocks, compute=compute)
    assert got.shape[-1] == 64 * blocks
    assert rel_err(got[..., :CIreal], ref) < (1e-5 if compute == "f32" else 2e-5)
    assert float(got[..., CIreal:].abs().sum()) == 0.0


def _make_pair(cin, cout, norm, device, settings=None, seed=0):
    from oracle.halfunet import HalfUNetRef
    from py4cast_amd.halfunet import HalfUNetMI355X, HalfUNetSettings

    torch.manual_seed(seed)
    ref = HalfUNetRef(cin, cout, norm=norm)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.GroupNorm)):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    model = HalfUNetMI355X(cin, cout, (32, 32), settings or HalfUNetSettings(norm=norm))
    model.load_state_dict(ref.state_dict(), strict=True)
    return ref, model.to(device)


def _ref_run(ref, x, gy, dt):
    xr = x.detach().clone().to(dt).requires_grad_(True)
    ref.train()
    yr = ref(xr.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    (yr * gy.to(dt)).sum().backward()
    return yr, xr.grad, dict(ref.named_parameters())


# floor of the parameter-gradient bar per draw: 2e-3 (test_model_gpu.py), or 1.5x what a 1e-6 relative perturbation of the first
# convolution's output alone moves the float64 oracle's parameter gradients by on that draw (tools/diagnostics/
# halfunet_grad_sensitivity.py: 1.2e-2, 9.8e-2, 1.7e-6, 9.6e-3 -- ReLU / max-pool ties flipping; wiring mistakes give O(0.1 .. 1)
# on every draw, and the input gradient keeps the 2e-3 bar everywhere)
@pytest.mark.parametrize("norm,cin,cout,H,W,grad_ch,floor", [("batch", 129, 60, 64, 64, None, 1.8e-2), ("batch", 189, 60, 32, 48, None, 1.5e-1),
                                                              ("group", 100, 21, 48, 32, None, 2e-3), ("batch", 89, 40, 32, 64, 80, 1.5e-2)])
def test_wide_halfunet_plan_matches_oracle(gpu_device, norm, cin, cout, H, W, grad_ch, floor):
    ref32, model = _make_pair(cin, cout, norm, gpu_device)
    if grad_ch is not None:
        model.grad_input_channels = grad_ch
    nchk = model.grad_input_channels
    assert nchk == (cin if grad_ch is None else grad_ch)
    ref64 = copy.deepcopy(ref32).double()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, H, W, cin, generator=g)
    gy = torch.randn(2, H, W, cout, generator=g)
    y64, dx64, p64 = _ref_run(ref64, x, gy, torch.float64)
    y32, dx32, p32 = _ref_run(ref32, x, gy, torch.float32)
    xg = x.to(gpu_device).requires_grad_(True)
    model.train()
    yg = model(xg)
    (yg * gy.to(gpu_device)).sum().backward()
    assert rel_err(yg, y64) < 1e-4
    # the gradient of every returned input channel, and zeros beyond
    assert rel_err(xg.grad[..., :nchk], dx64[..., :nchk]) < _noise_bar(rel_err(dx32[..., :nchk], dx64[..., :nchk]), 2e-3)
    assert float(xg.grad[..., nchk:].abs().sum()) == 0.0
    for name, p in model.named_parameters():
        assert rel_err(p.grad, p64[name].grad) < _noise_bar(rel_err(p32[name].grad, p64[name].grad), floor), name


@pytest.mark.parametrize("act", ["f32", "bf16"])
@pytest.mark.parametrize("cin,cout", [(129, 60), (189, 60)])
def test_wide_halfunet_bf16_tracks_oracle(gpu_device, cin, cout, act):
    """bf16 matrix cores with fp32 / bf16 storage (bf16 storage: the data gradient as one row-kernel launch per output block)."""
    from oracle.halfunet import HalfUNetRef
    from py4cast_amd.halfunet import HalfUNetMI355X, HalfUNetSettings

    torch.manual_seed(0)
    H, W = 64, 64
    ref = HalfUNetRef(cin, cout).double()
    model = HalfUNetMI355X(cin, cout, (H, W), HalfUNetSettings(compute_dtype="bf16", activation_dtype=act))
    model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    model = model.to(gpu_device).train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, H, W, cin, generator=g)
    gy = torch.randn(2, H, W, cout, generator=g)
    yr, dxr, pr = _ref_run(ref, x, gy, torch.float64)
    xg = x.to(gpu_device).requires_grad_(True)
    yg = model(xg)
    (yg * gy.to(gpu_device)).sum().backward()
    assert rel_err(yg, yr) < (8e-2 if act == "f32" else 0.1)   # the bars of test_model_gpu.py's bf16 plan tests
    for c0 in range(0, cin, 64):   # direction of the input gradient, per 64-channel output block of the data gradient
        a, b = xg.grad[..., c0:c0 + 64].detach().cpu().double().flatten(), dxr[..., c0:c0 + 64].flatten()
        assert float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.85, c0
    # (bf16 STORAGE rounds every activation and gradient map as well: at 189 inputs a 64-element norm-bias gradient drifts to a cosine
    # of ~0.82; a wrong block or channel offset gives ~0)
    bar = 0.85 if act == "f32" else 0.75
    for name, p in model.named_parameters():
        a, b = p.grad.detach().cpu().double().flatten(), pr[name].grad.flatten()
        assert float(torch.dot(a, b) / (a.norm() * b.norm())) > bar, name


@pytest.mark.parametrize("F,T", [(60, 2), (40, 3)])
def test_training_step_with_two_input_states_matches_oracle(gpu_device, F, T):
    """AutoRegressiveLightning with num_input_steps = 2: loss and BPTT gradients vs the float64 oracle.  At F = 40 (89 input
    channels) the state channels 64 .. 79 carry gradient between AR steps; at F = 60 the network has 129 input channels."""
    from helpers import make_batch, make_dataset_info, synthetic_case
    from oracle import losses as olosses
    from oracle import rollout as orollout
    from oracle.halfunet import HalfUNetRef
    from py4cast_amd.lightning import AutoRegressiveLightning

    T_in, Ff, Fs = 2, 5, 4
    case = synthetic_case(seed=5, B=2, T=T, T_in=T_in, H=32, W=32, F=F, Ff=Ff, Fs=Fs, border=2)
    info = make_dataset_info(case, Ff)
    torch.manual_seed(0)
    lm = AutoRegressiveLightning(
        {}, info, None, num_input_steps=T_in, num_pred_steps_train=T, batch_size=2, model_name="HalfUNet",
        losses=[{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}],
        training_strategy="scaled_ar",
    )
    assert lm.model.grad_input_channels >= T_in * F
    ref32 = HalfUNetRef(T_in * F + Fs + Ff, F)
    ref32.load_state_dict(lm.model.state_dict())
    ref64 = copy.deepcopy(ref32).double()
    lm = lm.to(gpu_device)
    lm.train()
    loss = lm.training_step(make_batch(case, gpu_device), 0)
    loss.backward()
    B = 2

    def run_ref(ref, dt):
        c = {k: v.to(dt) for k, v in case.items()}
        statics = c["statics"].unsqueeze(0).expand(B, *c["statics"].shape)
        interior = 1.0 - c["border_mask"]
        ref.train()
        pred = orollout.rollout(ref, c["inputs"], c["forcing"], c["outputs"], statics, c["border_mask"], interior,
                                c["diff_std"], c["diff_mean"], "scaled_ar", 1, False, "train", features_second=True)
        wts = olosses.weighted_loss_weights(c["state_weight"], c["diff_std"], "mse")
        l = olosses.training_loss(pred, c["outputs"], False, [("WeightedLoss", 1.0, dict(weights=wts, interior_mask=interior, kind="mse"))])
        l.backward()
        return l, dict(ref.named_parameters())

    l64, p64 = run_ref(ref64, torch.float64)
    l32, p32 = run_ref(ref32, torch.float32)
    assert abs(loss.item() - l64.item()) / abs(l64.item()) < 1e-4
    for name, p in lm.model.named_parameters():
        assert rel_err(p.grad, p64[name].grad) < _noise_bar(rel_err(p32[name].grad, p64[name].grad), 6e-2), name


@pytest.mark.parametrize("CIreal", [120, 189, 256])
def test_wide_data_grad_row_kernel_per_block(gpu_device, CIreal):
    """The plan's data gradient of the first convolution with bf16 storage: one row-kernel launch per 64-channel output block, block m
    reading rows 64m .. 64m+63 of the M_pad = 64 * blocks image and writing its columns of the 64 * blocks wide dx rows."""
    import ctypes

    from py4cast_amd import _lib as L
    from py4cast_amd import ops_model as om

    B, H, W = 2, 16, 128
    blocks = (CIreal + 63) // 64
    bf = om._compute("bf16")
    assert L.lib().p4c_conv_kernel_kind(bf, bf, 64, 3, B, H, W) == 2   # the row-streaming kernel
    g = torch.Generator().manual_seed(CIreal + 1)
    w = torch.randn(64, CIreal, 3, 3, generator=g) * 0.05
    dout = torch.randn(B, H, W, 64, generator=g).bfloat16()
    x = torch.zeros(B, CIreal, H, W, dtype=torch.float64, requires_grad=True)
    Fn.conv2d(x, _bf(w), padding=1).backward(dout.double().permute(0, 3, 1, 2))
    ref = _bf(x.grad.permute(0, 2, 3, 1))   # rounded once, on store
    wp = om.prep_weights(w.to(gpu_device), True, 64 * blocks, 64, compute="bf16")
    d = dout.to(gpu_device)
    out = torch.full((B, H, W, 64 * blocks), float("nan"), dtype=torch.bfloat16, device=gpu_device)
    blk = 9 * 64 * 64   # elements of one block's image
    for m in range(blocks):
        L.call("p4c_conv_fwd", L.ptr(d), bf, bf, 64, ctypes.c_void_p(wp.data_ptr() + m * blk * 2), 3, None, None, 0, None,
               ctypes.c_void_p(out.data_ptr() + m * 64 * 2), 64 * blocks, None, B, H, W, 1, L.stream(gpu_device))
    assert not torch.isnan(out).any()   # every column of the strided rows written
    assert rel_err(out[..., :CIreal], ref) < 1e-2   # one bf16 ulp where the fp32 sums round to different sides
    assert float(out[..., CIreal:].float().abs().sum()) == 0.0
