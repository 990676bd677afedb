"""UNETR++ (BASELINE configuration 5) on MI355X: the tall-skinny kernels against torch, the model against its float64 oracle
(parity unpinned: mfai is absent), a 6-step differential-AR rollout through the Lightning module, registry names."""
import numpy as np
import pytest
import torch

from helpers import make_batch, make_dataset_info, synthetic_case

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 6e-3)])
@pytest.mark.parametrize("B,H,N,d,e", [(2, 4, 1000, 8, 8), (1, 16, 4099, 16, 64), (2, 3, 257, 32, 32), (1, 2, 70, 64, 64), (2, 2, 5000, 12, 36), (1, 2, 300, 128, 128), (1, 3, 200, 128, 32)])
def test_tall_skinny_gram_and_apply(gpu_device, dtype, tol, B, H, N, d, e):
    """gram / apply on strided in-place views (slices of a (B,N,4,H,d) projection output) vs float64 matmuls, and their gradients
    (each kernel is the other's adjoint)."""
    from py4cast_amd import ops_ts as TS

    g = torch.Generator().manual_seed(N + d)
    big = torch.randn(B, N, 4, H, d, generator=g).to(gpu_device).to(dtype).requires_grad_(True)
    yfull = torch.randn(B, N, H, e, generator=g).to(gpu_device).to(dtype).requires_grad_(True)
    x = big[:, :, 1].permute(0, 2, 1, 3)             # (B,H,N,d) view with strides (N*4*H*d, d, 4*H*d, 1)
    y = yfull.permute(0, 2, 1, 3)
    assert not x.is_contiguous()
    m = torch.randn(B, H, d, e, generator=g).to(gpu_device).requires_grad_(True)
    G = TS.gram(x, y)
    O = TS.apply(x, m)
    xd, yd, md = x.detach().double(), y.detach().double(), m.detach().double()
    assert G.dtype == torch.float32 and _rel(G, xd.transpose(-1, -2) @ yd) < tol
    assert O.shape == (B, H, N, e) and O.permute(0, 2, 1, 3).is_contiguous() and _rel(O.float(), xd @ md) < tol
    wG = torch.randn(G.shape, generator=g).to(gpu_device)
    wO = torch.randn(B, N, H, e, generator=g).to(gpu_device).permute(0, 2, 1, 3)
    ((G * wG).sum() + (O.float() * wO).sum()).backward()
    dx_ref = yd @ wG.double().transpose(-1, -2) + wO.double() @ md.transpose(-1, -2)
    dy_ref = xd @ wG.double()
    dm_ref = xd.transpose(-1, -2) @ wO.double()
    btol = tol * 3
    assert _rel(big.grad[:, :, 1].permute(0, 2, 1, 3).float(), dx_ref) < btol
    assert float(big.grad[:, :, 0].abs().sum()) == 0.0
    assert _rel(yfull.grad.permute(0, 2, 1, 3).float(), dy_ref) < btol
    assert _rel(m.grad, dm_ref) < btol


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,N,d,e", [(2, 4, 1000, 32, 32), (2, 4, 515, 32, 64), (1, 4, 300, 64, 32), (1, 3, 257, 128, 128), (2, 4, 256, 256, 256),
                                       (1, 1, 100, 64, 8), (1, 2, 33, 8, 72), (1, 5, 64, 24, 40), (1, 4, 256, 256, 32)])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_apply_on_matrix_cores(gpu_device, B, H, N, d, e, out_dtype):
    """The matrix-core form of apply (csrc/tallskinny.hip: apply_mfma_kernel; bf16 token matrices, any width in one launch) against
    float64 on the same bf16-rounded operands (the small matrix rounded to bf16 as the kernel does), ragged token counts, head counts
    that do not fill a workgroup, in-place strided views, fp32 / bf16 outputs, and the accumulating form."""
    from py4cast_amd import _lib as L, ops_ts as TS

    g = torch.Generator().manual_seed(N * 7 + d + e)
    big = torch.randn(B, N, 4, H, d, generator=g).to(gpu_device).to(torch.bfloat16)
    x = big[:, :, 2].permute(0, 2, 1, 3)
    m = torch.randn(B, H, d, e, generator=g).to(gpu_device)
    assert TS._wide(x, torch.empty(B, N, H, e, dtype=out_dtype, device=gpu_device).permute(0, 2, 1, 3), d, e)
    O = TS._apply_raw(x, m, out_dtype)
    ref = x.double() @ m.to(torch.bfloat16).double()
    scale = float(ref.abs().max())
    err = float((O.double() - ref).abs().max()) / scale
    assert err < (1e-5 if out_dtype == torch.float32 else 4e-3), err
    # accumulate into what is there
    full = torch.randn(B, N + 3, H, e, generator=g).to(gpu_device).to(out_dtype)     # three guard rows behind each sample's tokens
    base, guard = full[:, :N].clone(), full[:, N:].clone()
    out = full[:, :N].permute(0, 2, 1, 3)
    L.call("p4c_ts_apply", L.ptr(x), L.dtype_code(x.dtype), *TS._strides(x), L.ptr(m), d * e, L.ptr(out), L.dtype_code(out_dtype), *TS._strides(out),
           B, H, N, d, e, 1, L.stream(x.device))
    ref2 = ref + base.permute(0, 2, 1, 3).double()
    err2 = float((out.double() - ref2).abs().max()) / scale
    assert err2 < (1e-5 if out_dtype == torch.float32 else 4e-3), err2
    assert torch.equal(full[:, N:], guard)       # stores are masked by token
    # the small matrix stored TRANSPOSED (p4c_ts_apply_mt: read as stored, no strided copy): bit-identical to the copy route
    mt = m.transpose(-1, -2).contiguous()                                       # (B,H,e,d) in memory
    assert TS._stored_transposed(mt.transpose(-1, -2)).data_ptr() == mt.data_ptr() and TS._stored_transposed(m) is None
    O2 = TS._apply_raw(x, mt.transpose(-1, -2), out_dtype)
    assert torch.equal(O2, O)
    out2 = base.clone().permute(0, 2, 1, 3)
    TS._apply_into(out2, x, mt.transpose(-1, -2), True)
    assert torch.equal(out2, out)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,N,d,e", [(2, 4, 5000, 32, 64), (2, 4, 256, 256, 256), (1, 5, 64, 24, 40), (1, 2, 33, 8, 72), (1, 3, 1000, 128, 32),
                                       (2, 4, 16384, 32, 32), (1, 1, 31, 64, 64)])
def test_gram_on_matrix_cores(gpu_device, B, H, N, d, e):
    """The matrix-core form of gram (csrc/tallskinny.hip: gram_mfma_kernel; bf16 token matrices, any width in one launch) against
    float64 on the same bf16 operands: ragged token counts (partial tiles, empty splits), widths that are not multiples of 32 or 64,
    in-place strided views; two runs are bit-identical (fixed-order sums, no atomics)."""
    from py4cast_amd import ops_ts as TS

    g = torch.Generator().manual_seed(N * 3 + d + e)
    big = torch.randn(B, N, 4, H, d, generator=g).to(gpu_device).to(torch.bfloat16)
    x = big[:, :, 3].permute(0, 2, 1, 3)
    y = torch.randn(B, N, H, e, generator=g).to(gpu_device).to(torch.bfloat16).permute(0, 2, 1, 3)
    assert TS._gram_wide(x, y)
    G = TS._gram_raw(x, y)
    ref = x.double().transpose(-1, -2) @ y.double()
    assert G.shape == (B, H, d, e) and G.dtype == torch.float32
    assert float((G.double() - ref).abs().max()) / float(ref.abs().max()) < 2e-5
    assert torch.equal(G, TS._gram_raw(x, y))


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,N,d,p", [(2, 16, 4099, 8, 64), (2, 4, 1000, 32, 64), (1, 16, 257, 64, 32), (1, 3, 70, 16, 24), (2, 16, 16384, 8, 64)])
def test_epa_spatial_branch_fused(gpu_device, B, H, N, d, p):
    """softmax(q Mq) VP^T as one node with the softmax / its adjoint in the apply epilogues (p4c_ts_apply_softmax) against float64 on
    the same bf16 q: output, and the gradients of q, Mq, VP^T."""
    from py4cast_amd import ops_ts as TS

    g = torch.Generator().manual_seed(N + d * p)
    big = torch.randn(B, N, 4, H, d, generator=g).to(gpu_device).to(torch.bfloat16).requires_grad_(True)
    q = big[:, :, 0].permute(0, 2, 1, 3)
    Mq = (torch.randn(B, H, d, p, generator=g) * 0.7).to(gpu_device).requires_grad_(True)
    VPt = torch.randn(B, H, p, d, generator=g).to(gpu_device).requires_grad_(True)
    assert TS.spatial_fused_ok(q, p)
    x = TS.epa_spatial(q, Mq, VPt)
    w = torch.randn(B, N, H, d, generator=g).to(gpu_device).permute(0, 2, 1, 3)
    (x.float() * w).sum().backward()
    qd = q.detach().double().requires_grad_(True)
    Md = Mq.detach().to(torch.bfloat16).double().requires_grad_(True)     # the kernel's operand: the small matrix rounded to bf16
    Vd = VPt.detach().double().requires_grad_(True)
    ref = (qd @ Md).softmax(dim=-1) @ Vd
    (ref * w.double()).sum().backward()
    assert x.shape == (B, H, N, d) and x.permute(0, 2, 1, 3).is_contiguous()
    assert _rel(x.float(), ref) < 8e-3
    assert _rel(big.grad[:, :, 0].permute(0, 2, 1, 3).float(), qd.grad) < 2e-2
    assert float(big.grad[:, :, 1:].abs().sum()) == 0.0
    assert _rel(Mq.grad, Md.grad) < 2e-2
    assert _rel(VPt.grad, Vd.grad) < 2e-2


def _pair(cin, cout, shape, dtype="f32", hidden=256, heads=4, linear=True, published=True):
    from oracle.unetrpp import UNetRPP as Oracle
    from py4cast_amd.unetrpp import UNetRPPMI355X, UNetRPPSettings

    torch.manual_seed(41)
    s = UNetRPPSettings(hidden_size=hidden, num_heads_encoder=heads, num_heads_decoder=4, depths=(2, 1, 1, 1), encoder_proj_sizes=(16, 16, 8, 4),
                        decoder_proj_size=16, linear_upsampling=linear, activation_dtype=dtype, published_block=published, conv8_dropout=0.0)
    model = UNetRPPMI355X(cin, cout, shape, s)
    with torch.no_grad():   # the published initialisation (gamma = 1e-6, zero positional embedding) would hide the attention path
        for n, p in model.named_parameters():
            if n.endswith("gamma"):
                p.fill_(0.5)
            elif n.endswith("pos_embed"):
                p.normal_(0, 0.1)
            elif "temperature" in n:
                p.uniform_(0.5, 1.5)
    oracle = Oracle(cin, cout, shape, hidden_size=hidden, num_heads_encoder=heads, num_heads_decoder=4, depths=(2, 1, 1, 1),
                    encoder_proj_sizes=(16, 16, 8, 4), decoder_proj_size=16, linear_upsampling=linear, published_block=published,
                    conv8_dropout=0.0).double()
    oracle.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()})   # (strict: the same keys)
    return model, oracle


@pytest.mark.parametrize("published", [True, False])
@pytest.mark.parametrize("linear", [True, False])
def test_unetrpp_matches_oracle(gpu_device, linear, published):
    """Both forms of the transformer block (UNetRPPSettings.published_block: as published / as mfai wraps it, and the restated one)
    against the oracle with the same switch.  Forward: always within the north-star bar.  Gradients: the network has ~10^6 LeakyReLU
    sites, and a pre-activation within fp32 rounding of zero (|z| ~ 1e-6, about one site per draw at this size) takes the other branch
    in fp32 than in the fp64 oracle: that site's gradient changes by O(1) and every gradient downstream by ~1e-3 -- a property of fp32,
    not of the kernels (tools/diagnostics/unetrpp_grad_probe6.py pins one such site: -2.8e-7 in fp64, +1.3e-6 in fp32).  So every draw
    is held to a loose sanity bound and AT LEAST FOUR OF THE SIX draws to the tight 1e-4 bar (a real defect fails every draw; the
    draws that miss it are reported with the tensor that moved most)."""
    H, W, cin, cout = 64, 96, 13, 5
    model, oracle = _pair(cin, cout, (H, W), linear=linear, published=published)
    model = model.to(gpu_device).train()
    oracle.train()
    ref = dict(oracle.named_parameters())
    seen = []
    for seed in range(42, 48):
        torch.manual_seed(seed)
        x, gy = torch.randn(2, H, W, cin), torch.randn(2, H, W, cout)
        model.zero_grad(set_to_none=True)
        oracle.zero_grad(set_to_none=True)
        xg = x.to(gpu_device).requires_grad_(True)
        y = model(xg)
        y.backward(gy.to(gpu_device))
        xr = x.double().requires_grad_(True)
        yr = oracle(xr)
        yr.backward(gy.double())
        assert y.shape == (2, H, W, cout)
        assert _rel(y, yr) < 1e-4                      # north-star bar: <= 1e-4 relative in fp32
        assert all(p.grad is not None for n, p in model.named_parameters())
        dx = _rel(xg.grad, xr.grad)
        worst = max((_rel(p.grad, ref[n].grad), n) for n, p in model.named_parameters())
        assert dx < 5e-2 and worst[0] < 2e-1, (seed, dx, worst)     # sanity on every draw (a branch flip moves small gradients by percents)
        seen.append((seed, dx, worst, dx < 1e-4 and worst[0] < 1e-4))
    tight = [s for s in seen if s[3]]
    assert len(tight) >= 4, f"only {len(tight)} of 6 draws met the 1e-4 gradient bar; the others (seed, dx, worst tensor): {[s[:3] for s in seen if not s[3]]}"


def test_unetrpp_published_block_has_the_published_state_dict(gpu_device):
    """published_block=True: the keys a checkpoint of the published code / mfai's wrapper carries -- ``conv8.1.*`` (conv8 =
    Sequential(Dropout2d, Conv2d)), ``epa_block.E.*`` AND ``epa_block.F.*`` (one Linear under two names) -- load strictly; the restated
    block has ``conv8.*`` and no ``F``; the channel dropout in front of conv8 is drawn in training mode only (p = conv8_dropout, 0.1 as
    published) and both forms compute the same function when x_SA's merge is undone by hand (the merge is the ONLY functional
    difference at p = 0)."""
    from py4cast_amd.unetrpp import UNetRPPMI355X, UNetRPPSettings

    kw = dict(hidden_size=128, num_heads_encoder=2, num_heads_decoder=2, depths=(1, 1, 1, 1), encoder_proj_sizes=(16, 16, 8, 4), decoder_proj_size=16,
              linear_upsampling=True)
    torch.manual_seed(7)
    pub = UNetRPPMI355X(9, 4, (64, 64), UNetRPPSettings(**kw))                      # defaults: published_block=True, conv8_dropout=0.1
    old = UNetRPPMI355X(9, 4, (64, 64), UNetRPPSettings(published_block=False, **kw))
    kp, ko = set(pub.state_dict()), set(old.state_dict())
    assert "stages.0.0.conv8.1.weight" in kp and "stages.0.0.conv8.1.bias" in kp and "stages.0.0.conv8.weight" not in kp
    assert "stages.0.0.epa_block.F.weight" in kp and "stages.0.0.epa_block.E.weight" in kp
    assert "stages.0.0.conv8.weight" in ko and not any(".F." in k for k in ko)
    assert len(list(pub.parameters())) == len(list(old.parameters()))              # E / F is ONE parameter pair
    assert pub.stages[0][0].epa_block.F is pub.stages[0][0].epa_block.E and pub.stages[0][0].conv8[0].p == 0.1
    # a published-form state dict loads strictly (also from the restated keys after renaming)
    sd = old.state_dict()
    ren = {k.replace(".conv8.", ".conv8.1."): v for k, v in sd.items()}
    ren.update({k.replace(".E.", ".F."): v for k, v in sd.items() if ".epa_block.E." in k})
    pub.load_state_dict(ren, strict=True)
    pub, old = pub.to(gpu_device), old.to(gpu_device)
    with torch.no_grad():
        for m in (pub, old):
            for n, p in m.named_parameters():
                if n.endswith("gamma"):
                    p.fill_(0.5)
    x = torch.randn(2, 64, 64, 9, generator=torch.Generator().manual_seed(8)).to(gpu_device)
    pub.eval(), old.eval()
    with torch.no_grad():
        ye1, ye2, yo = pub(x), pub(x), old(x)
    assert torch.equal(ye1, ye2)                                                   # eval: no draw
    assert float((ye1 - yo).abs().max()) > 1e-4                                     # the x_SA merge differs: another function
    pub.train()
    with torch.no_grad():
        torch.manual_seed(1); a = pub(x)
        torch.manual_seed(2); b = pub(x)
        torch.manual_seed(1); c = pub(x)
    assert not torch.equal(a, b) and torch.equal(a, c)                              # training: drawn, reproducible under the seed


def test_unetrpp_bf16_tracks_fp32(gpu_device):
    H, W, cin, cout = 64, 64, 13, 5
    model, oracle = _pair(cin, cout, (H, W), dtype="bf16")
    model = model.to(gpu_device).train()
    oracle.train()
    x = torch.randn(2, H, W, cin, generator=torch.Generator().manual_seed(3))
    y = model(x.to(gpu_device))
    assert y.dtype == torch.float32 and _rel(y, oracle(x.double())) < 5e-2


def test_unetrpp_six_step_diff_ar_rollout_through_lightning(gpu_device):
    """BASELINE configuration 5 in small: UNetRPP from the registry, 6-step differential AR (unetrpp.yaml with training_strategy
    diff_ar), fused update + loss per step, loss and gradients against the oracle network driven through the oracle rollout."""
    from oracle import losses as olosses
    from oracle import rollout as orollout
    from oracle.unetrpp import UNetRPP as Oracle
    from py4cast_amd.lightning import AutoRegressiveLightning
    from py4cast_amd.models import registry

    assert "UNetRPP" in registry and "UNetRPPMI355X" in registry
    H = W = 64
    F, Ff, T = 6, 5, 6
    case = synthetic_case(seed=51, B=2, T=T, H=H, W=W, F=F, Ff=Ff, border=0)
    info = make_dataset_info(case, Ff)
    settings = dict(hidden_size=128, num_heads_encoder=2, num_heads_decoder=2, depths=[1, 1, 1, 1], encoder_proj_sizes=[16, 16, 8, 4],
                    decoder_proj_size=16, linear_upsampling=True, attention_code="torch", conv8_dropout=0.0)   # published block, no draw
    torch.manual_seed(52)
    lm = AutoRegressiveLightning(settings, info, None, num_input_steps=1, num_pred_steps_train=T, batch_size=2, model_name="UNetRPP",
                                 losses=[{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}],
                                 training_strategy="diff_ar").to(gpu_device).train()
    with torch.no_grad():
        for n, p in lm.model.named_parameters():
            if n.endswith("gamma"):
                p.fill_(0.5)
    loss = lm.training_step(make_batch(case, gpu_device), 0)
    loss.backward()
    m = lm.model
    oracle = Oracle(m.in_channels, m.out_channels, (H, W), hidden_size=128, num_heads_encoder=2, num_heads_decoder=2, depths=(1, 1, 1, 1),
                    encoder_proj_sizes=(16, 16, 8, 4), decoder_proj_size=16, linear_upsampling=True, conv8_dropout=0.0).double().train()
    oracle.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.cpu() for k, v in m.state_dict().items()})
    c = {k: (v.double() if v.is_floating_point() else v) for k, v in case.items()}
    statics = c["statics"].unsqueeze(0).expand(2, *c["statics"].shape)
    interior = 1.0 - c["border_mask"]
    pred = orollout.rollout(oracle, c["inputs"], c["forcing"], c["outputs"], statics, c["border_mask"], interior, None, None,
                            training_strategy="diff_ar")
    w = olosses.weighted_loss_weights(c["state_weight"], c["diff_std"], "mse")
    ref = olosses.weighted_loss(pred, c["outputs"], torch.ones_like(pred), w, interior, "mse").mean()
    ref.backward()
    assert abs(loss.item() - ref.item()) / abs(ref.item()) < 2e-4
    rg = dict(oracle.named_parameters())
    worst = max((_rel(p.grad, rg[n].grad), n) for n, p in m.named_parameters())
    assert worst[0] < 3e-2, worst     # six chained networks in fp32 (BatchNorm batch statistics inside): see test_model_gpu.py on BPTT noise


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 8e-3)])
@pytest.mark.parametrize("CI,ks,H,W", [(69, 3, 24, 40), (64, 3, 16, 32), (69, 1, 12, 36), (10, 3, 8, 8)])
def test_conv_nhwc_autograd_node(gpu_device, dtype, tol, CI, ks, H, W):
    """ops_model.conv_nhwc (forward, data gradient for ALL input channels, weight gradient on the native kernels) vs torch's conv2d
    in float64 on the same (rounded) operands -- the route UNetRPP's full-resolution 64-channel residual blocks take."""
    import torch.nn.functional as Fn

    from py4cast_amd import ops_model as om

    g = torch.Generator().manual_seed(CI + ks)
    x = torch.randn(2, H, W, CI, generator=g).to(dtype)
    w = torch.randn(64, CI, ks, ks, generator=g) * 0.1
    gy = torch.randn(2, H, W, 64, generator=g).to(dtype)
    xg = x.to(gpu_device).requires_grad_(True)
    wg = w.to(gpu_device).requires_grad_(True)
    y = om.conv_nhwc(xg, wg)
    y.backward(gy.to(gpu_device))
    xr = x.double().requires_grad_(True)
    wr = (w.to(dtype).double() if dtype == torch.bfloat16 else w.double()).requires_grad_(True)
    yr = Fn.conv2d(xr.permute(0, 3, 1, 2), wr, padding=ks // 2).permute(0, 2, 3, 1)
    yr.backward(gy.double())
    assert y.shape == (2, H, W, 64) and y.dtype == dtype
    assert _rel(y.float(), yr) < tol
    assert xg.grad.shape == x.shape and _rel(xg.grad.float(), xr.grad) < tol
    assert _rel(wg.grad, wr.grad) < (1e-4 if dtype == torch.float32 else 2e-3)


@pytest.mark.parametrize("shape", [(2, 16, 8, 64), (2, 16, 16, 64), (1, 16, 32, 64), (2, 16, 64, 32), (2, 4, 16, 64)])
def test_epa_small_matrices_native_node(gpu_device, shape):
    """ops_ts.epa_small (p4c_epa_small_fwd / _bwd: norms, channel-attention softmax and the scaled token projection of an EPA block in
    one launch each way) against the torch op chain it replaces, in float64, values and every gradient."""
    from py4cast_amd import ops_ts as TS

    B, H, d, p = shape
    g = torch.Generator().manual_seed(11)
    q, k = torch.randn(B, H, 200, d, generator=g), torch.randn(B, H, 200, d, generator=g)
    G0, Gq0, Gk0 = q.transpose(-1, -2) @ k, q.transpose(-1, -2) @ q, k.transpose(-1, -2) @ k
    KP0 = torch.randn(B, H, d, p, generator=g)
    t10, t20 = torch.rand(H, 1, 1, generator=g) + 0.5, torch.rand(H, 1, 1, generator=g) + 0.5
    dAt, dMq = torch.randn(B, H, d, d, generator=g), torch.randn(B, H, d, p, generator=g)

    def chain(G, Gq, Gk, KP, t1, t2):
        nq = torch.diagonal(Gq, dim1=-2, dim2=-1).clamp_min(0).sqrt().clamp_min(1e-12)
        nk = torch.diagonal(Gk, dim1=-2, dim2=-1).clamp_min(0).sqrt().clamp_min(1e-12)
        A = (G / (nq.unsqueeze(-1) * nk.unsqueeze(-2)) * t1).softmax(dim=-1)
        return A.transpose(-1, -2), KP / nq.unsqueeze(-1) * t2

    ref_in = [t.double().requires_grad_(True) for t in (G0, Gq0, Gk0, KP0, t10, t20)]
    At_r, Mq_r = chain(*ref_in)
    (At_r * dAt.double()).sum().add((Mq_r * dMq.double()).sum()).backward()
    dev_in = [t.to(gpu_device).requires_grad_(True) for t in (G0, Gq0, Gk0, KP0, t10, t20)]
    At, Mq = TS.epa_small(*dev_in)
    ((At * dAt.to(gpu_device)).sum() + (Mq * dMq.to(gpu_device)).sum()).backward()
    assert _rel(At.detach().cpu(), At_r.detach()) < 2e-6 and _rel(Mq.detach().cpu(), Mq_r.detach()) < 2e-6
    for name, a, b in zip(("G", "Gq", "Gk", "KP", "t1", "t2"), dev_in, ref_in):
        assert _rel(a.grad.cpu(), b.grad) < 2e-5, name


@pytest.mark.parametrize("shape", [(2, 16, 1000, 8), (2, 8, 4096, 16), (1, 4, 777, 32), (2, 2, 300, 64)])
def test_gram_with_column_norms(gpu_device, shape):
    """ops_ts.gram_norms (p4c_ts_gram_norms): q^T k and the squared column norms of q and k from one pass, values and gradients against
    float64 on the same bf16 operands; and epa_small fed with the norms' diagonals equals epa_small fed with the full grams."""
    from py4cast_amd import ops_ts as TS

    B, H, N, d = shape
    g = torch.Generator().manual_seed(13)
    big = torch.randn(B, N, 4, H, d, generator=g).bfloat16().to(gpu_device).requires_grad_(True)
    q, k = big[:, :, 0].permute(0, 2, 1, 3), big[:, :, 1].permute(0, 2, 1, 3)        # strided views, as in EPA
    G, nq2, nk2 = TS.gram_norms(q, k)
    wG, wq, wk = torch.randn(B, H, d, d, generator=g), torch.randn(B, H, d, generator=g), torch.randn(B, H, d, generator=g)
    ((G * wG.to(gpu_device)).sum() + (nq2 * wq.to(gpu_device)).sum() + (nk2 * wk.to(gpu_device)).sum()).backward()
    ref = big.detach().double().cpu().requires_grad_(True)
    qr, kr = ref[:, :, 0].permute(0, 2, 1, 3), ref[:, :, 1].permute(0, 2, 1, 3)
    Gr, nqr, nkr = qr.transpose(-1, -2) @ kr, (qr * qr).sum(dim=2), (kr * kr).sum(dim=2)
    ((Gr * wG.double()).sum() + (nqr * wq.double()).sum() + (nkr * wk.double()).sum()).backward()
    assert _rel(G.detach().cpu(), Gr.detach()) < 1e-5 and _rel(nq2.detach().cpu(), nqr.detach()) < 1e-5 and _rel(nk2.detach().cpu(), nkr.detach()) < 1e-5
    assert _rel(big.grad.float().cpu()[:, :, :2], ref.grad[:, :, :2]) < 8e-3     # bf16 gradient rows
    assert not big.grad[:, :, 2:].any()                                             # (v slices untouched by this node)
    # the small-matrix node: diagonals in == full grams in
    KP = torch.randn(B, H, d, 64, generator=g).to(gpu_device)
    t1, t2 = (torch.rand(H, 1, 1, generator=g) + 0.5).to(gpu_device), (torch.rand(H, 1, 1, generator=g) + 0.5).to(gpu_device)
    Gd = G.detach()
    a1, m1 = TS.epa_small(Gd, nq2.detach(), nk2.detach(), KP, t1, t2)
    a2, m2 = TS.epa_small(Gd, torch.diag_embed(nq2.detach()), torch.diag_embed(nk2.detach()), KP, t1, t2)
    assert torch.equal(a1, a2) and torch.equal(m1, m2)


def test_unetrpp_takes_its_input_straight_from_build_x(gpu_device):
    """``rollout_input_format`` (bf16 flavour): bf16 rows zero-padded to 32 channels from build_x, bf16 back -- same loss, same gradients
    up to the bf16 rounding of the summed input gradient, against the fp32-rows route."""
    from py4cast_amd.lightning import AutoRegressiveLightning

    H = W = 64
    F, Ff, T = 6, 5, 3
    case = synthetic_case(seed=61, B=2, T=T, H=H, W=W, F=F, Ff=Ff, border=0)
    info = make_dataset_info(case, Ff)
    settings = dict(hidden_size=128, num_heads_encoder=2, num_heads_decoder=2, depths=[1, 1, 1, 1], encoder_proj_sizes=[16, 16, 8, 4],
                    decoder_proj_size=16, linear_upsampling=True, attention_code="torch", activation_dtype="bf16", conv8_dropout=0.0)
    torch.manual_seed(62)
    lm = AutoRegressiveLightning(settings, info, None, num_input_steps=1, num_pred_steps_train=T, batch_size=2, model_name="UNetRPP",
                                 losses=[{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}],
                                 training_strategy="diff_ar").to(gpu_device).train()
    assert lm.model.rollout_input_format == (torch.bfloat16, 32)
    seen = []
    hook = lm.model.register_forward_pre_hook(lambda mod, args: seen.append((args[0].dtype, args[0].shape[-1])))
    out = {}
    for use in (True, False):
        lm.use_rollout_input_format = use
        lm.zero_grad(set_to_none=True)
        loss = lm.training_step(make_batch(case, gpu_device), 0)
        loss.backward()
        out[use] = (loss.item(), torch.cat([p.grad.float().flatten() for p in lm.model.parameters()]))
    hook.remove()
    assert seen[:T] == [(torch.bfloat16, 32)] * T and seen[T:] == [(torch.float32, lm.model.in_channels)] * T
    (la, ga), (lb, gb) = out[True], out[False]
    # (inside the rollout the 6-feature output head runs on the row-GEMM kernel, padded to 8 outputs, instead of the library's GEMM:
    # the bf16 outputs differ by a rounding here and there)
    assert abs(la - lb) / abs(lb) < 1e-3, (la, lb)
    cos = float((ga.double() * gb.double()).sum() / (ga.double().norm() * gb.double().norm()))
    assert cos > 0.999, cos


@pytest.mark.parametrize("N,hidden,heads,proj", [(256, 64, 4, 16), (1024, 128, 16, 64), (4096, 128, 4, 32), (16384, 128, 16, 64), (4096, 256, 16, 64),
                                                 (1024, 512, 4, 64), (256, 1024, 16, 32)])     # (128-wide heads; 512 / 1024 channels per token)
def test_epa_core_as_one_node(gpu_device, monkeypatch, diag_library, N, hidden, heads, proj):
    """The attention between the projections as ONE autograd node (ops_ts.epa_core: dq / dk / dv written straight into the gradient of
    the qkvv projection) against the same module composed of separate nodes: identical output (same kernels, same order), gradients
    equal up to the bf16 rounding of sums taken in another order."""
    from py4cast_amd.unetrpp import EPA

    torch.manual_seed(N + heads)
    m = EPA(N, hidden, proj, heads).to(gpu_device)
    with torch.no_grad():
        m.temperature.uniform_(0.5, 1.5)
        m.temperature2.uniform_(0.5, 1.5)
    x0 = torch.randn(2, N, hidden, generator=torch.Generator().manual_seed(7)).to(gpu_device).to(torch.bfloat16)
    w = torch.randn(2, N, hidden, generator=torch.Generator().manual_seed(8)).to(gpu_device)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("P4C_EPA_CORE", flag)
        m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = m(x)
        (y.float() * w).sum().backward()
        out[flag] = (y.detach().float(), x.grad.float(), {n: p.grad.float().clone() for n, p in m.named_parameters()})
    (ya, xa, ga), (yb, xb, gb) = out["1"], out["0"]
    print("epa_core vs composed: output", _rel(ya, yb), "dx", _rel(xa, xb), {n: round(_rel(ga[n], gb[n]), 5) for n in ga})
    # (round 6: the node's token-axis projection accumulates and adds its bias in fp32 -- the composed module's is the library's bf16
    #  GEMM result; with 128-wide heads the composed module has no fused small-matrix node either: other roundings, not other kernels)
    assert _rel(ya, yb) < 5e-3
    assert _rel(xa, xb) < 2e-2
    for n in ga:
        assert _rel(ga[n], gb[n]) < 2e-2, n
    # round 6: the token-axis projection E = F and its adjoints run on the tall-skinny kernels with k / v_sa read in place
    # (ops_ts._token_proj_native: gram over all channels of a sample + one launch for splits / bias; apply into dqkvv; apply +
    # transposing sum for dW).  The gather + library GEMM route of rounds 3-5 (diagnostic switch) gives the same node.
    from py4cast_amd import ops_ts as TS

    probe = torch.empty(2, N, 4, heads, hidden // heads, dtype=torch.bfloat16, device=gpu_device)
    assert TS._token_proj_native(probe, proj)
    monkeypatch.setenv("P4C_EPA_CORE", "1")
    monkeypatch.setenv("P4C_EPA_LIB_PROJ", "1")
    assert not TS._token_proj_native(probe, proj)
    m.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    y = m(x)
    (y.float() * w).sum().backward()
    gl = {n: p.grad.float().clone() for n, p in m.named_parameters()}
    print("native vs library projection: output", _rel(ya, y.detach().float()), "dx", _rel(xa, x.grad.float()),
          {n: round(_rel(ga[n], gl[n]), 5) for n in ga})
    # (the library route rounds KP / VP to bf16 -- the GEMM's output type -- before the small-matrix kernel reads them: 2^-9 per element)
    assert _rel(ya, y.detach().float()) < 5e-3 and _rel(xa, x.grad.float()) < 2e-2
    for n in ga:
        assert _rel(ga[n], gl[n]) < 2e-2, n
    monkeypatch.delenv("P4C_EPA_LIB_PROJ")
    # with a gradient buffer on E.weight (FlatDDP / the trainer allocate them) the weight gradient is ADDED into it by the transposing
    # sum itself (ops_gemm.GRADS_IN_PLACE): twice the gradient after two backward passes, nothing through autograd
    m.zero_grad(set_to_none=False)
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        (m(x).float() * w).sum().backward()
    assert _rel(m.E.weight.grad.float(), 2 * ga["E.weight"]) < 2e-3


@pytest.mark.parametrize("N,hidden,heads,proj", [
    (16384, 128, 16, 64), (4096, 256, 16, 64), (1024, 512, 16, 64), (256, 1024, 16, 32),     # the benchmark's encoder stages
    (1024, 512, 4, 64), (4096, 256, 4, 64), (16384, 128, 4, 64),                              # its decoders
    (256, 64, 4, 16), (520, 64, 8, 8), (64, 128, 1, 64)])                                      # small: 16 / 8 / 128-wide heads
def test_epa_core_against_float64(gpu_device, N, hidden, heads, proj):
    """ops_ts.epa_core against the float64 EPA algebra of tests/unetrpp_nodes.epa_node on the same bf16 qkvv (E's weight read as its
    bf16 image; the stored S and dL rounded as the module docstring there names): outputs and every gradient at the node bars of
    tests/test_unetrpp_nodes_gpu.py -- temperatures other than 1, a non-zero E bias.  Then the sink route: with E.weight.grad present the
    node adds its weight gradient into it, bit for bit prefill + the gradient autograd received."""
    import unetrpp_nodes as UN
    from py4cast_amd import ops_ts as TS

    B, d = 2, hidden // heads
    g = torch.Generator(device=gpu_device).manual_seed(N * 7 + hidden + heads)
    qkvv = torch.randn(B, N, 4, heads, d, device=gpu_device, generator=g).to(torch.bfloat16).requires_grad_(True)
    W = ((torch.rand(proj, N, device=gpu_device, generator=g) * 2 - 1) / N ** 0.5).requires_grad_(True)
    bias = (torch.rand(proj, device=gpu_device, generator=g) - 0.5).requires_grad_(True)
    t1 = (torch.rand(heads, 1, 1, device=gpu_device, generator=g) * 2.5 + 0.5).requires_grad_(True)
    t2 = (torch.rand(heads, 1, 1, device=gpu_device, generator=g) * 2.5 + 0.5).requires_grad_(True)
    # incoming gradients as the network hands them: token-major (B, N, heads, d) memory seen as (B, heads, N, d)
    dxs = torch.randn(B, N, heads, d, device=gpu_device, generator=g).to(torch.bfloat16).permute(0, 2, 1, 3)
    dxc = torch.randn(B, N, heads, d, device=gpu_device, generator=g).to(torch.bfloat16).permute(0, 2, 1, 3)
    assert TS.epa_core_ok(qkvv, proj)
    x_sa, x_ca = TS.epa_core(qkvv, W, bias, t1, t2)
    torch.autograd.backward([x_sa, x_ca], [dxs, dxc])
    ref = UN.epa_node(qkvv, W, bias, t1, t2, dxs, dxc)
    got = UN.epa_measure(x_sa, x_ca, qkvv.grad, W.grad, bias.grad, t1.grad, t2.grad, ref)
    print(f"\nepa_core {N}x{hidden} heads {heads} p {proj}:", ", ".join(f"{k} {v:.1e}" for k, v in got.items()))
    bad = {k: f"{v:.2e} > {UN.EPA_BARS[k]:.0e}" for k, v in got.items() if not v <= UN.EPA_BARS[k]}
    assert not bad, bad
    # sink route: E.weight.grad pre-filled, the node's transposing sum adds the finished fp32 sum into it
    gW = W.grad.clone()
    prefill = torch.randn(proj, N, device=gpu_device, generator=g)
    W.grad = prefill.clone()
    x_sa, x_ca = TS.epa_core(qkvv, W, bias, t1, t2)
    torch.autograd.backward([x_sa, x_ca], [dxs, dxc])
    assert torch.equal(W.grad, prefill + gW)


def test_unetrpp_bf16_step_makes_no_library_convolution_and_tracks_the_oracle(gpu_device, monkeypatch):
    """Round 5: the 128 ... 1024-channel convolutions, batch norms and projections of the bf16 flavour run on csrc/gemm.hip.  A forward
    + backward at the yaml's head / stage structure must not reach ops_model.library_conv2d nor torch's batch norm, its output must
    track the float64 oracle at the bf16 bar, its parameter gradients must point the oracle's way (cosine), and a rerun must
    reproduce every gradient bit for bit."""
    import py4cast_amd.ops_model as OM

    calls = {"conv": 0, "bn": 0}
    real_conv, real_bn = OM.library_conv2d, torch.nn.functional.batch_norm
    monkeypatch.setattr(OM, "library_conv2d", lambda *a, **k: (calls.__setitem__("conv", calls["conv"] + 1), real_conv(*a, **k))[1])
    monkeypatch.setattr(torch.nn.functional, "batch_norm", lambda *a, **k: (calls.__setitem__("bn", calls["bn"] + 1), real_bn(*a, **k))[1])
    H, W, cin, cout = 64, 64, 16, 8
    model, oracle = _pair(cin, cout, (H, W), dtype="bf16", hidden=256, heads=4)
    model = model.to(gpu_device).train()
    oracle.train()
    x = torch.randn(2, H, W, cin, generator=torch.Generator().manual_seed(5))
    gy = torch.randn(2, H, W, cout, generator=torch.Generator().manual_seed(6))

    def run():
        model.zero_grad(set_to_none=True)
        y = model(x.to(gpu_device))
        y.backward(gy.to(gpu_device))
        return y.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}

    y, grads = run()
    assert calls == {"conv": 0, "bn": 0}, calls
    yr = oracle(x.double())
    yr.backward(gy.double())
    assert _rel(y, yr) < 5e-2
    ref = dict(oracle.named_parameters())
    cos = {n: float(torch.nn.functional.cosine_similarity(g.double().flatten().cpu(), ref[n].grad.flatten(), dim=0)) for n, g in grads.items()}
    low = {n: c for n, c in cos.items() if c < 0.9}
    assert len(low) <= len(cos) // 20, low          # bf16 against float64: nearly all tensors well aligned
    assert sum(cos.values()) / len(cos) > 0.97
    y2, grads2 = run()
    assert torch.equal(y, y2) and all(torch.equal(grads[n], grads2[n]) for n in grads)
