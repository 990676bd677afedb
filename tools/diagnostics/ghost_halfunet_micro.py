"""HalfUNet with Ghost blocks (use_ghost), the native bf16 route against the module route it replaces, on the GPU --
profiles/ghost_halfunet.txt:

1. the A/B distances of tests/test_ghost_native_gpu.py (2 x 48 x 64, training forward + backward, eval) and, at the timed size, of the
   training-mode output: both routes against the float64 oracle on the same state dict;
2. the four kernels of csrc/ghost.hip at 2 x 512 x 512 x 64 bf16 and the coarser levels, each against the sequence it replaces;
3. the whole training step (training_step + backward through AutoRegressiveLightning: scaled_ar, T = 3, B = 2, 512 x 512 x 60, 5 forcings,
   4 statics) on the native route and on the retained module route (P4C_GHOST_MODULES=1, diagnostic library).

Device events; every shape warmed up; the sides alternate inside one process, median of 5 rounds with the rounds listed; no profiler.  A
kernel call is tens of microseconds behind as much host work, so the kernel sides are captured into HIP graphs (one stream) of
CALLS_PER_GRAPH calls and the replays are timed.

    python tools/diagnostics/ghost_halfunet_micro.py [--out profiles/ghost_halfunet.txt] [--rounds 5] [--size 512]
"""
import argparse
import copy
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CALLS_PER_GRAPH = 10
BF16 = {"compute_dtype": "bf16", "activation_dtype": "bf16"}
MSE = [{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}]
OUT = []


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    OUT.append(line)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(CALLS_PER_GRAPH):
            fn()
    return graph.replay


def compare(title, sides, rounds, nbytes):
    """{name: fn}: the sides' graph replays in alternating rounds of 10; TB/s on the FIRST side's algorithmic bytes"""
    replays = {k: captured(f) for k, f in sides.items()}
    for r in replays.values():
        timed(r, 3)
    runs = {k: [] for k in sides}
    for _ in range(rounds):
        for k, r in replays.items():
            runs[k].append(timed(r, 10) / CALLS_PER_GRAPH)
    base = None
    say(title)
    for k, v in runs.items():
        t = statistics.median(v)
        base = t if base is None else base
        say(f"  {k}: {1e6 * t:.1f} us ({nbytes / t / 1e12:.2f} TB/s on {nbytes / 1e6:.1f} MB; rounds {' '.join(f'{1e6 * x:.1f}' for x in v)})"
            f" | x{t / base:.2f}")


def kernels(dev, rounds, size):
    from py4cast_amd import _lib as L

    lib, st = L.lib(), L.stream
    g = torch.Generator(device=dev).manual_seed(0)
    bf = torch.bfloat16
    B = 2
    w = (0.3 * torch.randn(32, 9, device=dev, generator=g)).contiguous()
    for k in range(5):
        H = W = size >> k
        n = B * H * W
        prim = torch.randn(B, H, W, 32, device=dev, generator=g).to(bf)
        full = torch.randn(B, H, W, 64, device=dev, generator=g).to(bf)
        dz = torch.randn(B, H, W, 64, device=dev, generator=g).to(bf)
        out, out2, dprim = torch.empty_like(full), torch.empty_like(full), torch.empty_like(prim)
        stats = torch.empty(lib.p4c_ghost_tail_blocks(B, H, W), 2, 64, device=dev)
        istats = torch.empty(lib.p4c_inorm_blocks(n, 64), 2, 64, device=dev)
        wpart = torch.empty(lib.p4c_ghost_tail_bwd_blocks(B, H, W), 32, 9, device=dev)
        opart = torch.empty(lib.p4c_ghost_dw_wgrad_blocks(B, H, W), 32, 9, device=dev)

        def k1():
            L.call("p4c_ghost_tail_fwd", L.ptr(prim), 32, L.ptr(w), L.ptr(out), 64, L.ptr(stats), L.BF16, B, H, W, st())

        def k1_old():
            L.call("p4c_ghost_dw_fwd", L.ptr(full), L.ptr(w), L.ptr(out2), L.BF16, B, H, W, st())
            L.call("p4c_inorm_reduce", L.ptr(out2), None, None, None, None, 1.0, L.ptr(istats), L.BF16, 1, n, 64, st())

        def k2():
            L.call("p4c_ghost_tail_bwd", L.ptr(dz), L.ptr(prim), 32, L.ptr(w), L.ptr(dprim), 32, L.ptr(wpart), L.BF16, B, H, W, st())

        def k2_old():
            L.call("p4c_ghost_dw_bwd_data", L.ptr(dz), L.ptr(w), L.ptr(out2), L.BF16, B, H, W, st())
            L.call("p4c_ghost_dw_wgrad", L.ptr(full), L.ptr(dz), L.ptr(opart), L.BF16, B, H, W, st())

        compare(f"K1 ghost tail forward, {B}x{H}x{W}", {"p4c_ghost_tail_fwd": k1, "p4c_ghost_dw_fwd + p4c_inorm_reduce": k1_old}, rounds,
                2 * n * (32 + 64))
        compare(f"K2 ghost tail backward, {B}x{H}x{W}", {"p4c_ghost_tail_bwd": k2, "p4c_ghost_dw_bwd_data + p4c_ghost_dw_wgrad": k2_old}, rounds,
                2 * n * (64 + 32 + 32))
    H = W = size
    maps = [torch.randn(B, H >> k, W >> k, 64, device=dev, generator=g).to(bf) for k in range(5)]
    dS = torch.randn(B, H, W, 64, device=dev, generator=g).to(bf)
    S = torch.empty_like(dS)
    chain = [torch.empty_like(dS) for _ in range(2)]
    tx = [torch.empty(B, H, W >> k, 64, device=dev) for k in (1, 2, 3, 4)]          # (fp32: the x pass's sums)
    da = [torch.empty(B, H >> k, W >> k, 64, device=dev, dtype=bf) for k in (1, 2, 3, 4)]

    def k3():
        L.call("p4c_halfunet_merge_fwd", *[L.ptr(a) for a in maps], L.ptr(S), L.BF16, B, H, W, 64, st())

    def k3_three():       # (p4c_upsample_bilinear_fwd serves scales up to 8: levels 1..3 only, a LOWER bound of a four-launch chain)
        src = maps[0]
        for k in (1, 2, 3):
            dst = chain[k % 2]
            L.call("p4c_upsample_bilinear_fwd", L.ptr(maps[k]), L.ptr(src), L.ptr(dst), B, H >> k, W >> k, 64, 1 << k, st())
            src = dst

    def k3_torch():       # the module route's code
        s = maps[0].float()
        for k in range(1, 5):
            s = s + F.interpolate(maps[k].permute(0, 3, 1, 2).float(), scale_factor=2 ** k, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        return s.to(bf)

    def k4():
        L.call("p4c_halfunet_merge_bwd", L.ptr(dS), *[L.ptr(t) for t in tx], *[L.ptr(t) for t in da], L.BF16, B, H, W, 64, st())

    def k4_three():       # levels 1..3 of the four separate adjoints (scale 16 is not served): a LOWER bound of the four launches
        for k in (1, 2, 3):
            L.call("p4c_upsample_bilinear_bwd", L.ptr(dS), L.ptr(da[k - 1]), B, H >> k, W >> k, 64, 1 << k, st())

    dSn = dS.permute(0, 3, 1, 2).float()

    def k4_torch():       # the module route's backward: four upsample_bilinear2d_backward on fp32 maps
        return [torch.ops.aten.upsample_bilinear2d_backward(dSn, [H, W], [B, 64, H >> k, W >> k], False, None, None) for k in (1, 2, 3, 4)]

    n = B * H * W
    coarse = sum(a.numel() for a in maps[1:])
    compare(f"K3 decoder merge forward, {B}x{H}x{W}x64",
            {"p4c_halfunet_merge_fwd": k3, "three p4c_upsample_bilinear_fwd with skip (levels 1..3 only)": k3_three,
             "F.interpolate + add, fp32 maps (module route)": k3_torch}, rounds, 2 * (2 * n * 64 + coarse))
    compare(f"K4 decoder merge adjoint, {B}x{H}x{W}x64",
            {"p4c_halfunet_merge_bwd (x pass + y pass)": k4, "three p4c_upsample_bilinear_bwd (levels 1..3 only)": k4_three,
             "four upsample_bilinear2d_backward, fp32 maps (module route)": k4_torch}, rounds,
            2 * (n * 64 + coarse) + 2 * 4 * sum(t.numel() for t in tx))


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double().to(got.device)
    return float((got - ref).norm() / ref.norm())


def distances(dev):
    import test_ghost_native_gpu as T

    H, W, cin, cout = 48, 64, 21, 12
    native, module, ref = T.ghost_models(dev, H, W, cin, cout)
    x = torch.randn(2, H, W, cin, generator=torch.Generator().manual_seed(10))
    gy = torch.randn(2, H, W, cout, generator=torch.Generator().manual_seed(11))
    want = T.oracle_train_then_eval(ref, x, gy)
    got_n = T.train_then_eval(native, x, gy, dev)
    os.environ["P4C_GHOST_MODULES"] = "1"
    got_m = T.train_then_eval(module, x, gy, dev)
    del os.environ["P4C_GHOST_MODULES"]
    say(f"distance from the float64 oracle at 2x{H}x{W}, {cin} -> {cout} channels (norm-wise relative; native route / module route):")
    for k in want:
        dn, dm = T.rel_err(got_n[k], want[k]), T.rel_err(got_m[k], want[k])
        say(f"  {k}: {dn:.4e} / {dm:.4e} (ratio {dn / dm:.3f})")


def whole_step(dev, rounds, size):
    from helpers import make_batch, make_dataset_info, synthetic_case
    from oracle.halfunet import HalfUNetRef
    from py4cast_amd.lightning import AutoRegressiveLightning

    case = synthetic_case(seed=3, B=2, T=3, H=size, W=size, F=60, Ff=5, Fs=4, border=0)
    info = make_dataset_info(case, 5)
    torch.manual_seed(1)
    lm = AutoRegressiveLightning({"use_ghost": True, **BF16}, info, None, num_pred_steps_train=3, batch_size=2, model_name="HalfUNet", losses=MSE,
                                 training_strategy="scaled_ar").to(dev).train()
    assert lm.model.ghost_native
    batch = make_batch(case, dev)
    state = copy.deepcopy(lm.state_dict())

    def step():
        lm.zero_grad(set_to_none=True)
        loss = lm.training_step(batch, 0)
        loss.backward()
        return loss

    def side(module_route):
        if module_route:
            os.environ["P4C_GHOST_MODULES"] = "1"
        else:
            os.environ.pop("P4C_GHOST_MODULES", None)

    # outputs at the timed size: one training-mode forward of each route against the float64 oracle (on the GPU) on the same state dict
    m = lm.model
    x = torch.randn(2, size, size, m.in_channels, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    ref = HalfUNetRef(m.in_channels, m.out_channels, use_ghost=True).double()
    ref.load_state_dict({k: v.double().cpu() if v.is_floating_point() else v.cpu() for k, v in m.state_dict().items()})
    ref = ref.to(dev).train()
    with torch.no_grad():
        side(False)
        yn = m(x)
        lm.load_state_dict(state)
        side(True)
        ym = m(x)
        lm.load_state_dict(state)
        say(f"training-mode output at 2x{size}x{size}, {m.in_channels} -> {m.out_channels} channels: native against module route, norm-wise "
            f"relative {rel(yn, ym):.4e}")
        try:
            want = ref(x.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
            dn, dm = rel(yn, want), rel(ym, want)
            say(f"  distance from the float64 oracle: native {dn:.4e} / module {dm:.4e} (ratio {dn / dm:.3f})")
            del want
        except RuntimeError as e:          # (the library may not serve a float64 convolution of this size)
            say(f"  distance from the float64 oracle at this size: not measured ({str(e).splitlines()[0][:120]})")
    del ref, yn, ym
    losses = {}
    for mr in (False, True):          # warm-up of both routes at the timed shape
        side(mr)
        for _ in range(2):
            losses[mr] = float(step().detach())
        lm.load_state_dict(state)
    runs = {False: [], True: []}
    for _ in range(rounds):
        for mr in (False, True):
            side(mr)
            runs[mr].append(timed(step, 2))
    side(False)
    say(f"whole step (training_step + backward, scaled_ar, T = 3, B = 2, {size}x{size}x60 + 5 forcings + 4 statics, bf16, eager, generic "
        f"per-step rollout): loss after warm-up native {losses[False]:.6f} / module {losses[True]:.6f}")
    for mr, name in ((False, "native route"), (True, "module route (P4C_GHOST_MODULES=1: the parent's code)")):
        v = runs[mr]
        say(f"  {name}: {1e3 * statistics.median(v):.1f} ms (rounds {' '.join(f'{1e3 * t:.1f}' for t in v)})")
    say(f"  module / native = x{statistics.median(runs[True]) / statistics.median(runs[False]):.2f}; native faster in every round: "
        f"{all(a < b for a, b in zip(runs[False], runs[True]))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ghost_halfunet.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ghost_halfunet_micro.py measures on the GPU"
    from py4cast_amd import _lib as L

    dev = torch.device("cuda:0")
    say(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; kernel sources sha {L.kernel_sources_sha16()}")
    with L.use_diagnostic_library():           # (P4C_GHOST_MODULES is a diagnostic switch)
        distances(dev)
        kernels(dev, args.rounds, args.size)
        whole_step(dev, args.rounds, args.size)
    with open(args.out, "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
