"""HalfUNet with Ghost blocks (use_ghost), the native bf16 route: the kernels of csrc/ghost.hip against float64 (torch ops in double on the
same stored operands), then the network -- against the float64 oracle next to the retained module route (P4C_GHOST_MODULES=1, diagnostic
library), the profile of a training step, the Lightning module and an auto-padded grid."""
import copy

import pytest
import torch
import torch.nn.functional as F

from helpers import make_batch, make_dataset_info, synthetic_case

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("diag_library")]   # (P4C_GHOST_MODULES selects the module route: diagnostic build)

MSE = [{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}]
BF16 = {"compute_dtype": "bf16", "activation_dtype": "bf16"}

# tail kernels: tiles of th x 64 pixels, th = 1 for maps this small (8, 4 or 2 rows once that leaves every CU 8 workgroups).  (1,7,33) is
# narrower than one tile, (2,16,24) too, (2,40,72) crosses tile borders in both directions with a ragged last tile in W, (3,64,64) is
# full tiles only; (1,512,512) is the smallest map that takes a taller tile (th = 2 on 256 CUs), several workgroups' worth of tiles each
TAIL_SHAPES = [(1, 7, 33), (2, 16, 24), (2, 40, 72), (3, 64, 64), (1, 512, 512)]
DTYPES = [(torch.float32, 1e-6), (torch.bfloat16, 8e-3)]
MERGE_SHAPES = [(1, 16, 16), (2, 32, 48), (1, 64, 32)]


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def max_err(got, ref):
    """largest deviation over the largest reference magnitude"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max())


def tail_operands(B, H, W, dtype, dev):
    g = torch.Generator().manual_seed(1000 * H + W)
    prim = (torch.randn(B, H, W, 32, generator=g) + 0.5).to(dtype)        # (a mean the statistics have to find)
    w = torch.randn(32, 1, 3, 3, generator=g) * 0.3
    dz = torch.randn(B, H, W, 64, generator=g).to(dtype)
    return prim.to(dev), w.to(dev), dz.to(dev)


def tail_fwd_raw(prim_map, ld, w, out, want_stats=True):
    from py4cast_amd import _lib as L

    B, H, W, _ = out.shape
    stats = torch.full((L.lib().p4c_ghost_tail_blocks(B, H, W), 2, 64), float("nan"), device=out.device) if want_stats else None
    L.call("p4c_ghost_tail_fwd", L.ptr(prim_map), ld, L.ptr(w.reshape(32, 9).contiguous()), L.ptr(out), 64, L.ptr(stats), L.dtype_code(out.dtype),
           B, H, W, L.stream())
    return stats


@pytest.mark.parametrize("dtype,tol", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H,W", TAIL_SHAPES)
def test_ghost_tail_forward(gpu_device, dtype, tol, B, H, W):
    """p4c_ghost_tail_fwd (tiles of th x 64 pixels, see TAIL_SHAPES): the primary half is a bit copy (out of place) or untouched (in place), the cheap half is
    the depthwise 3x3 of float64 within the bars of test_ghost_depthwise_kernels, the statistics are the sums of the STORED map to 1e-4,
    and a second run is bit-identical."""
    prim, w, _ = tail_operands(B, H, W, dtype, gpu_device)
    out = torch.full((B, H, W, 64), float("nan"), device=gpu_device, dtype=dtype)
    stats = tail_fwd_raw(prim, 32, w, out)
    inplace = torch.full((B, H, W, 64), float("nan"), device=gpu_device, dtype=dtype)
    inplace[..., :32] = prim
    stats_in = tail_fwd_raw(inplace, 64, w, inplace)
    ref = F.conv2d(prim.double().cpu().permute(0, 3, 1, 2), w.double().cpu(), padding=1, groups=32).permute(0, 2, 3, 1)
    for got, st in ((out, stats), (inplace, stats_in)):
        assert torch.equal(got[..., :32], prim)
        assert torch.isfinite(got.float()).all() and torch.isfinite(st).all()
        err = rel_err(got[..., 32:], ref)
        stored = got.double().cpu().reshape(-1, 64)
        sums = st.double().cpu().sum(dim=0)
        e1, e2 = rel_err(sums[0], stored.sum(dim=0)), rel_err(sums[1], stored.square().sum(dim=0))
        print(f"tail_fwd {dtype} {(B, H, W)}: cheap {err:.3e} sum {e1:.3e} sumsq {e2:.3e}")
        assert err < tol
        assert e1 < 1e-4 and e2 < 1e-4
    assert torch.equal(out, inplace) and torch.equal(stats, stats_in)
    again = torch.empty_like(out)
    stats2 = tail_fwd_raw(prim, 32, w, again)
    assert torch.equal(out, again) and torch.equal(stats, stats2)
    # without statistics the map is the same
    nostat = torch.empty_like(out)
    tail_fwd_raw(prim, 32, w, nostat, want_stats=False)
    assert torch.equal(out, nostat)


@pytest.mark.parametrize("dtype,tol", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H,W", TAIL_SHAPES)
def test_ghost_tail_backward(gpu_device, dtype, tol, B, H, W):
    """p4c_ghost_tail_bwd against float64 autograd of [prim | depthwise3x3(prim)], and against p4c_ghost_dw_bwd_data's channels 0..31;
    prim at pixel stride 32 and 64; bit-identical reruns."""
    from py4cast_amd import _lib as L

    prim, w, dz = tail_operands(B, H, W, dtype, gpu_device)
    wf = w.reshape(32, 9).contiguous()
    nb = L.lib().p4c_ghost_tail_bwd_blocks(B, H, W)

    def run(pm, ld):
        dprim = torch.full((B, H, W, 32), float("nan"), device=gpu_device, dtype=dtype)
        wpart = torch.full((nb, 32, 9), float("nan"), device=gpu_device)
        L.call("p4c_ghost_tail_bwd", L.ptr(dz), L.ptr(pm), ld, L.ptr(wf), L.ptr(dprim), 32, L.ptr(wpart), L.dtype_code(dtype), B, H, W, L.stream())
        return dprim, wpart

    dprim, wpart = run(prim, 32)
    wide = torch.full((B, H, W, 64), float("nan"), device=gpu_device, dtype=dtype)
    wide[..., :32] = prim
    dprim64, wpart64 = run(wide, 64)
    assert torch.equal(dprim, dprim64) and torch.equal(wpart, wpart64)
    again = run(prim, 32)
    assert torch.equal(dprim, again[0]) and torch.equal(wpart, again[1])

    pr = prim.double().cpu().requires_grad_(True)
    wr = w.double().cpu().requires_grad_(True)
    z = torch.cat([pr, F.conv2d(pr.permute(0, 3, 1, 2), wr, padding=1, groups=32).permute(0, 2, 3, 1)], dim=-1)
    z.backward(dz.double().cpu())
    old = torch.empty(B, H, W, 64, device=gpu_device, dtype=dtype)
    L.call("p4c_ghost_dw_bwd_data", L.ptr(dz), L.ptr(wf), L.ptr(old), L.dtype_code(dtype), B, H, W, L.stream())
    e_d, e_w, e_old = rel_err(dprim, pr.grad), rel_err(wpart.sum(dim=0).view(32, 1, 3, 3), wr.grad), rel_err(dprim, old[..., :32])
    print(f"tail_bwd {dtype} {(B, H, W)}: dprim {e_d:.3e} dw {e_w:.3e} vs ghost_dw_bwd_data {e_old:.3e}")
    assert torch.isfinite(dprim.float()).all() and torch.isfinite(wpart).all()
    assert e_d < tol
    assert e_w < max(tol, 2e-5)
    assert e_old < tol


def test_ghost_tail_node_gradients(gpu_device):
    """ops_ghost_native.ghost_tail: the weight gradient reaches the parameter through autograd when it has no gradient buffer yet and
    is added into the buffer in place afterwards (ops_gemm._sink): the second backward doubles it exactly."""
    from py4cast_amd.ops_ghost_native import ghost_tail

    prim, w, dz = tail_operands(2, 16, 24, torch.bfloat16, gpu_device)
    wp = torch.nn.Parameter(w.clone())
    pg = prim.clone().requires_grad_(True)
    z, stats = ghost_tail(pg, wp)
    assert stats is not None and not stats.requires_grad
    z.backward(dz)
    g1, d1 = wp.grad.clone(), pg.grad.clone()
    z2, _ = ghost_tail(pg, wp)
    z2.backward(dz)
    assert torch.equal(wp.grad, 2 * g1) and torch.equal(pg.grad, 2 * d1)
    z3, none = ghost_tail(prim, wp, want_stats=False)
    assert none is None and torch.equal(z3, z)


def merge_operands(B, H, W, dtype, dev):
    g = torch.Generator().manual_seed(H * W)
    maps = [torch.randn(B, H >> k, W >> k, 64, generator=g).to(dtype).to(dev) for k in range(5)]
    dS = torch.randn(B, H, W, 64, generator=g).to(dtype).to(dev)
    return maps, dS


def merge_ref(maps):
    """float64 on the CPU: the sum of F.interpolate's bilinear up-samplings, leaves that require a gradient"""
    leaves = [a.double().cpu().requires_grad_(True) for a in maps]
    s = leaves[0]
    for k in range(1, 5):
        s = s + F.interpolate(leaves[k].permute(0, 3, 1, 2), scale_factor=2 ** k, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    return leaves, s


def top_of_binade(t, ref_max):
    """t scaled (and rounded to its dtype again) so that a result of magnitude ref_max, linear in t, lands at 1.995 x a power of two.
    One bf16 rounding of a value v is off by at most half an ulp = 2^(e-8) for |v| in [2^e, 2^(e+1)), so over the largest magnitude
    m 2^e it is at most 2^-8 / m: only with m >= 1.99 is that the 2^-9 + 1e-5 the bf16 bar of these tests asks for.  The operands are
    therefore scaled to put max|ref| there (the tests assert it)."""
    e = torch.floor(torch.log2(torch.tensor(float(ref_max))))
    return (t.double() * (1.995 * 2.0 ** float(e) / float(ref_max))).to(t.dtype)


BF16_ROUNDING = 2.0 ** -9 + 1e-5


def mantissa(v):
    v = float(v)
    return v / 2.0 ** float(torch.floor(torch.log2(torch.tensor(v))))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H,W", MERGE_SHAPES)
def test_halfunet_merge_forward(gpu_device, dtype, B, H, W):
    """p4c_halfunet_merge_fwd against float64 (F.interpolate, align_corners=False): deviation over max|ref| within 1e-6 in fp32 storage
    and within one rounding of the fp32 sum, 2^-9 + 1e-5, in bf16 (operands scaled as `top_of_binade` explains); at (1,16,16) the
    coarsest level is 1 x 1 and every tap clamps.  Bit-identical reruns."""
    from py4cast_amd.ops_ghost_native import halfunet_merge

    maps, _ = merge_operands(B, H, W, dtype, gpu_device)
    if dtype == torch.bfloat16:
        peak = merge_ref(maps)[1].detach().abs().max()
        maps = [top_of_binade(a, peak) for a in maps]
    ref = merge_ref(maps)[1].detach()
    if dtype == torch.bfloat16:
        assert mantissa(ref.abs().max()) >= 1.99
    S = halfunet_merge(*maps)
    e_f = max_err(S, ref)
    print(f"merge_fwd {dtype} {(B, H, W)}: {e_f:.3e}")
    assert S.dtype == dtype and S.shape == maps[0].shape and torch.isfinite(S.float()).all()
    assert e_f <= (1e-6 if dtype == torch.float32 else BF16_ROUNDING)
    assert torch.equal(S, halfunet_merge(*maps))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H,W", MERGE_SHAPES)
def test_halfunet_merge_adjoint(gpu_device, dtype, B, H, W):
    """p4c_halfunet_merge_bwd against float64 autograd of the F.interpolate sum, the bars of the forward test: each level is judged on a
    dS scaled for THAT level's max|ref| in bf16 (`top_of_binade`; the four gradients are linear in dS, each with its own largest
    element).  fp32 storage: <merge(a), dS> = sum_k <a_k, da_k> to 1e-5.  da_0 is dS itself.  Bit-identical reruns."""
    from py4cast_amd.ops_ghost_native import halfunet_merge

    maps, dS0 = merge_operands(B, H, W, dtype, gpu_device)

    def both(dS):
        leaves_g = [a.clone().requires_grad_(True) for a in maps]
        S = halfunet_merge(*leaves_g)
        S.backward(dS)
        leaves, ref = merge_ref(maps)
        ref.backward(dS.double().cpu())
        return S, [a.grad for a in leaves_g], [a.grad for a in leaves]

    S, got, want = both(dS0)
    assert torch.equal(got[0], dS0)                 # the full-resolution level's gradient is dS itself
    if dtype == torch.float32:
        e_b = [max_err(g, w) for g, w in zip(got[1:], want[1:])]
        print(f"merge_bwd {dtype} {(B, H, W)}: " + " ".join(f"{e:.3e}" for e in e_b))
        assert all(g.shape == a.shape for g, a in zip(got, maps)) and max(e_b) <= 1e-6, e_b
        lhs = float((S.detach().double() * dS0.double()).sum())
        rhs = sum(float((a.double() * g.double()).sum()) for a, g in zip(maps, got))
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)
    else:
        for k in range(1, 5):
            dS = top_of_binade(dS0, want[k].abs().max())
            _, got_k, want_k = both(dS)
            assert mantissa(want_k[k].abs().max()) >= 1.99
            e = max_err(got_k[k], want_k[k])
            print(f"merge_bwd {dtype} {(B, H, W)} level {k}: {e:.3e}")
            assert got_k[k].dtype == dtype and got_k[k].shape == maps[k].shape and e <= BF16_ROUNDING, (k, e)
    again = both(dS0)[1]
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_halfunet_merge_rejects_unsupported_shapes(gpu_device):
    from py4cast_amd import _lib as L
    from py4cast_amd.ops_ghost_native import halfunet_merge

    dev = gpu_device
    maps = [torch.zeros(1, 24 >> k, 32 >> k, 64, device=dev) for k in range(5)]          # H = 24 is no multiple of 16
    with pytest.raises(L.P4CError):
        halfunet_merge(*maps)
    with pytest.raises(L.P4CError):
        halfunet_merge(*[torch.zeros(1, 32 >> k, 32 >> k, 32, device=dev) for k in range(5)])      # 32 channels
    ok = [torch.zeros(1, 32 >> k, 32 >> k, 64, device=dev) for k in range(5)]
    out = torch.zeros_like(ok[0])
    ptrs = [L.ptr(a) for a in ok]
    for H, W, C in ((24, 32, 64), (32, 40, 64), (32, 32, 32), (0, 32, 64)):       # the C entry points themselves (they return before a launch)
        with pytest.raises(L.P4CError, match="p4c_halfunet_merge_fwd"):
            L.call("p4c_halfunet_merge_fwd", *ptrs, L.ptr(out), L.F32, 1, H, W, C, L.stream())
        with pytest.raises(L.P4CError, match="p4c_halfunet_merge_bwd"):
            L.call("p4c_halfunet_merge_bwd", L.ptr(out), *ptrs[1:], *ptrs[1:], L.F32, 1, H, W, C, L.stream())
    with pytest.raises(L.P4CError, match="bad dtype"):
        L.call("p4c_halfunet_merge_fwd", *ptrs, L.ptr(out), 77, 1, 32, 32, 64, L.stream())
    with pytest.raises(L.P4CError, match="ld_prim"):
        L.call("p4c_ghost_tail_fwd", L.ptr(out), 48, L.ptr(out), L.ptr(out), 64, None, L.F32, 1, 32, 32, L.stream())


# ------------------------------------------------------------------------------------------------ network
def ghost_models(dev, H, W, cin, cout, seed=9, **kw):
    """(native-route model, module-route model, float64 oracle) on one state dict"""
    from oracle.halfunet import HalfUNetRef
    from py4cast_amd.halfunet import HalfUNetMI355X, HalfUNetSettings

    torch.manual_seed(seed)
    model = HalfUNetMI355X(cin, cout, (H, W), HalfUNetSettings(use_ghost=True, **BF16, **kw))
    assert model.ghost_native and model.module_path and model.native_rollout is None
    ref = HalfUNetRef(cin, cout, use_ghost=True).double()
    assert set(model.state_dict()) == set(ref.state_dict())
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()})
    other = copy.deepcopy(model)
    return model.to(dev), other.to(dev), ref


def train_then_eval(model, x, gy, dev):
    model.train()
    xg = x.to(dev).requires_grad_(True)
    y = model(xg)
    y.backward(gy.to(dev))
    grads = torch.cat([p.grad.detach().double().reshape(-1).cpu() for _, p in sorted(model.named_parameters())])
    stats = torch.cat([b.detach().double().reshape(-1).cpu() for _, b in sorted(model.named_buffers()) if b.dtype.is_floating_point])
    model.eval()
    with torch.no_grad():
        ye = model(x.to(dev))
    return {"output": y.detach(), "input gradient": xg.grad, "parameter gradients": grads, "running statistics": stats, "eval output": ye}


def oracle_train_then_eval(ref, x, gy):
    ref.train()
    xr = x.double().requires_grad_(True)
    yr = ref(xr.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    yr.backward(gy.double())
    grads = torch.cat([p.grad.reshape(-1) for _, p in sorted(ref.named_parameters())])
    stats = torch.cat([b.reshape(-1).double() for _, b in sorted(ref.named_buffers()) if b.dtype.is_floating_point])
    ref.eval()
    with torch.no_grad():
        ye = ref(x.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    return {"output": yr.detach(), "input gradient": xr.grad, "parameter gradients": grads, "running statistics": stats, "eval output": ye}


def test_ghost_native_network_against_float64_next_to_the_module_route(gpu_device, monkeypatch):
    """B = 2, 48 x 64, 21 -> 12 channels, the weights and inputs of test_ghost_halfunet_matches_oracle_and_trains: training forward +
    backward, then eval, on the native bf16 route and on the retained module route (P4C_GHOST_MODULES=1), both against the float64 oracle
    on the same state dict.  The two routes store the same maps in bf16 and differ in the order of fp32 sums, so each native distance
    (norm-wise relative) must be <= 1.5 x the module route's; a wrong tap or statistic moves it to O(1).
    Measured on an MI355X (native / module, also in profiles/ghost_halfunet.txt): output 3.556e-2 / 3.454e-2, input gradient 0.3998 /
    0.4063, parameter gradients 0.3862 / 0.3923, running statistics 1.488e-4 / 1.459e-4, eval output 8.07e-3 / 8.16e-3 -- ratios
    0.98 ... 1.03 (the gradients of this random, untrained network sit at 0.4 from float64 on either route: bf16 maps through twelve
    batch norms)."""
    dev = gpu_device
    H, W, cin, cout = 48, 64, 21, 12
    native, module, ref = ghost_models(dev, H, W, cin, cout)
    x = torch.randn(2, H, W, cin, generator=torch.Generator().manual_seed(10))
    gy = torch.randn(2, H, W, cout, generator=torch.Generator().manual_seed(11))
    want = oracle_train_then_eval(ref, x, gy)
    got_n = train_then_eval(native, x, gy, dev)
    monkeypatch.setenv("P4C_GHOST_MODULES", "1")
    got_m = train_then_eval(module, x, gy, dev)
    monkeypatch.delenv("P4C_GHOST_MODULES")
    dist = {k: (rel_err(got_n[k], want[k]), rel_err(got_m[k], want[k])) for k in want}
    for k, (dn, dm) in dist.items():
        print(f"ghost network, {k}: native {dn:.4e} module {dm:.4e} ratio {dn / dm:.3f}")
    assert not torch.equal(got_n["output"], got_m["output"])          # (two routes, not one route twice)
    for k, (dn, dm) in dist.items():
        assert dn <= 1.5 * dm, (k, dn, dm)
    assert all(int(b) == 1 for n, b in native.named_buffers() if n.endswith("num_batches_tracked"))


def test_ghost_native_route_of_a_training_step(gpu_device):
    """2 x 64 x 64, 21 input channels: the profile of a training step holds no library convolution / norm / pool / interpolate / cat
    and no host read-back, it holds the four kernels of csrc/ghost.hip, and a second step from the same state is bit-identical."""
    from torch.profiler import ProfilerActivity, profile

    from py4cast_amd.halfunet import HalfUNetMI355X, HalfUNetSettings

    dev = gpu_device
    torch.manual_seed(0)
    m = HalfUNetMI355X(21, 12, (64, 64), HalfUNetSettings(use_ghost=True, **BF16)).to(dev).train()
    x = torch.randn(2, 64, 64, 21, device=dev)
    state = copy.deepcopy(m.state_dict())

    def step():
        m.load_state_dict(state)
        m.zero_grad(set_to_none=True)
        y = m(x)
        loss = y.float().square().mean()
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), y.detach().clone(), [p.grad.detach().clone() for p in m.parameters()]

    step()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        l1, y1, g1 = step()
    names = [e.name for e in prof.events()]
    low = [n.lower() for n in names]
    for bad in ("miopen", "batch_norm", "max_pool", "upsample_bilinear"):
        hits = [n for n in low if bad in n and not n.startswith("p4c")]
        assert not hits, (bad, hits[:5])
    banned = ("aten::cat", "aten::convolution", "aten::native_batch_norm", "aten::item", "aten::_local_scalar_dense")
    hits = [n for n in names if n in banned or n.startswith("aten::max_pool2d") or n.startswith("aten::upsample_bilinear2d")]
    assert not hits, sorted(set(hits))
    kernels = " ".join(low)
    for k in ("ghost::tail_fwd_kernel", "ghost::tail_bwd_kernel", "ghost::merge_fwd_kernel", "ghost::merge_bwd_pass_kernel"):
        assert k in kernels, k
    l2, y2, g2 = step()
    assert torch.isfinite(l1) and torch.equal(l1, l2) and torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_ghost_native_through_the_lightning_module(gpu_device, monkeypatch):
    """scaled_ar, T = 2, 32 x 32 (the level-5 map is 2 x 2), F = 12, bf16, the generic per-step rollout: a finite loss, a gradient on
    every parameter, and the loss within 1e-2 relative of the module route's (the bf16 bar of tests/test_inter_steps_rollout_gpu.py)."""
    from py4cast_amd.lightning import AutoRegressiveLightning

    case = synthetic_case(seed=13, B=2, T=2, H=32, W=32, F=12, Ff=5, Fs=4, border=0)
    info = make_dataset_info(case, 5)

    def run():
        torch.manual_seed(31)
        lm = AutoRegressiveLightning({"use_ghost": True, **BF16}, info, None, num_pred_steps_train=2, batch_size=2, model_name="HalfUNet",
                                     losses=MSE, training_strategy="scaled_ar").to(gpu_device)
        assert lm.model.ghost_native and lm.model.native_rollout is None
        loss = lm.training_step(make_batch(case, gpu_device), 0)
        loss.backward()
        assert bool(torch.isfinite(loss))
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in lm.model.parameters())
        return float(loss.detach())

    native = run()
    monkeypatch.setenv("P4C_GHOST_MODULES", "1")
    module = run()
    print(f"ghost lightning loss: native {native:.6f} module {module:.6f}")
    assert abs(native - module) <= 1e-2 * abs(module)


def test_ghost_native_autopad(gpu_device, monkeypatch):
    """40 x 72 with autopad_enabled: padded to 48 x 80 (centred), run on the native route, cropped; the shape is kept and the output's
    distance from the float64 oracle (on the padded input, cropped) is <= 1.5 x the module route's."""
    dev = gpu_device
    H, W, cin, cout = 40, 72, 21, 12
    native, module, ref = ghost_models(dev, H, W, cin, cout, seed=5, autopad_enabled=True)
    x = torch.randn(2, H, W, cin, generator=torch.Generator().manual_seed(6))
    top, bottom, left, right = native.padding_for(H, W)
    assert (top, bottom, left, right) == (4, 4, 4, 4)
    ref.train()
    with torch.no_grad():
        xp = F.pad(x.double(), (0, 0, left, right, top, bottom))
        want = ref(xp.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)[:, top: top + H, left: left + W]
    native.train(), module.train()
    xg = x.to(dev).requires_grad_(True)
    yn = native(xg)
    yn.float().square().mean().backward()
    assert yn.shape == (2, H, W, cout) and xg.grad.shape == x.shape and bool(torch.isfinite(xg.grad).all())
    monkeypatch.setenv("P4C_GHOST_MODULES", "1")
    with torch.no_grad():
        ym = module(x.to(dev))
    dn, dm = rel_err(yn, want), rel_err(ym, want)
    print(f"ghost autopad output: native {dn:.4e} module {dm:.4e}")
    assert ym.shape == yn.shape and not torch.equal(yn, ym)
    assert dn <= 1.5 * dm, (dn, dm)
