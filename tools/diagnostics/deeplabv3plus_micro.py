"""DeepLabV3+'s two passes (csrc/deeplabplus.hip) against what they replace, on the GPU, at the bench operands (2 x 512 x 512: the
stride-16 map is 2 x 32 x 32 x 512, the decoder 2 x 128 x 128 x (256 + 48)) -- profiles/deeplabv3plus_kernels.txt:

1. the ASPP's depthwise 3x3 at rates (12, 24, 36), forward + backward (data and weight gradients): ONE three-rate launch each way against
   three single-rate launches of the same kernel, and against three F.conv2d(groups=C, padding=r, dilation=r) on the library under bf16
   (channels-last memory) with their autograd backward;
2. up_cat (bilinear align_corners x4 + concatenation, forward + backward) against upsample_bilinear_ac + torch.cat and their backward.

A call is tens of microseconds of kernel time behind as much host work, so each side's 20 forward + backward calls are captured into one
HIP graph (one stream) and the replays are timed with device events: warm-up, then the median of 5 alternating rounds of 10 replays, in a
fresh process.

    python tools/diagnostics/deeplabv3plus_micro.py [--rounds 5] [--skip-library]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CALLS_PER_GRAPH = 20
RATES = (12, 24, 36)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def captured(fn):
    """CALLS_PER_GRAPH calls of fn as one HIP graph on one stream; returns the replay"""
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


def compare(sides, rounds):
    """{name: fn} -> {name: (median seconds per call, runs)}, the sides' graph replays timed in alternating rounds of 10"""
    replays = {k: captured(f) for k, f in sides.items()}
    for r in replays.values():
        timed(r, 3)
    runs = {k: [] for k in sides}
    for _ in range(rounds):
        for k, r in replays.items():
            runs[k].append(timed(r, 10) / CALLS_PER_GRAPH)
    return {k: (statistics.median(v), v) for k, v in runs.items()}


def report(title, res, nbytes):
    base = next(iter(res.values()))[0]
    print(title, flush=True)
    for k, (t, runs) in res.items():
        print(f"  {k}: {1e6 * t:.1f} us per call ({nbytes / t / 1e12:.2f} TB/s on the fused side's {nbytes / 1e6:.1f} MB; runs "
              f"{' '.join(f'{1e6 * v:.1f}' for v in runs)}) | x{t / base:.2f} of the first", flush=True)


def depthwise_micro(dev, rounds, library):
    from py4cast_amd.deeplabv3plus import depthwise3x3_dilated

    B, H, W, C = 2, 32, 32, 512
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, H, W, C, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    ws = [(0.3 * torch.randn(C, 1, 3, 3, device=dev, generator=g)).requires_grad_(True) for _ in RATES]
    dys = [torch.randn(B, H, W, C, device=dev, generator=g).to(torch.bfloat16) for _ in RATES]

    def clear():
        x.grad = None
        for w in ws:
            w.grad = None

    def one_launch():
        clear()
        torch.autograd.backward(list(depthwise3x3_dilated(x, ws, RATES)), dys)

    def three_launches():
        clear()
        ys = [depthwise3x3_dilated(x, [w], (d,))[0] for w, d in zip(ws, RATES)]
        torch.autograd.backward(ys, dys)

    sides = {"one three-rate launch each way": one_launch, "three single-rate launches each way": three_launches}
    if library:
        wb = [w.detach().to(torch.bfloat16).requires_grad_(True) for w in ws]
        dyn = [dy.permute(0, 3, 1, 2) for dy in dys]       # (the same memory: channels-last)

        def lib():
            x.grad = None
            for w in wb:
                w.grad = None
            xn = x.permute(0, 3, 1, 2)
            torch.autograd.backward([F.conv2d(xn, w, padding=d, dilation=d, groups=C) for w, d in zip(wb, RATES)], dyn)

        sides["three F.conv2d(groups=C, dilation=r) under bf16"] = lib
    one_launch()
    ref = x.grad.clone()
    three_launches()
    print(f"dx of the one-launch route against the sum of three launches' dx (autograd adds those in bf16): max abs diff "
          f"{float((ref.float() - x.grad.float()).abs().max()):.3e} of {float(ref.float().abs().max()):.3e}")
    # forward x + R y; data gradient R dy + dx; weight gradient x + R dy
    nbytes = 2 * x.numel() * ((1 + len(RATES)) * 2 + 1 + len(RATES))
    report(f"depthwise 3x3, rates {RATES}, x {B}x{H}x{W}x{C}, forward + backward: {CALLS_PER_GRAPH} calls per HIP-graph replay, median of "
           f"{rounds} alternating rounds of 10 replays", compare(sides, rounds), nbytes)


def up_cat_micro(dev, rounds):
    from py4cast_amd.deeplabv3 import upsample_bilinear_ac
    from py4cast_amd.deeplabv3plus import up_cat

    B, h, w, Ca, Cs, s = 2, 32, 32, 256, 48, 4
    g = torch.Generator(device=dev).manual_seed(1)
    a = torch.randn(B, h, w, Ca, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    skip = torch.randn(B, s * h, s * w, Cs, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    dout = torch.randn(B, s * h, s * w, Ca + Cs, device=dev, generator=g).to(torch.bfloat16)

    def fused():
        a.grad = skip.grad = None
        up_cat(a, skip, s).backward(dout)

    def separate():
        a.grad = skip.grad = None
        torch.cat([upsample_bilinear_ac(a, s), skip], dim=-1).backward(dout)

    fused()
    ga, gs = a.grad.clone(), skip.grad.clone()
    separate()
    assert torch.equal(ga, a.grad) and torch.equal(gs, skip.grad)
    nbytes = 2 * 2 * (a.numel() + skip.numel() + dout.numel())
    report(f"up_cat, a {B}x{h}x{w}x{Ca} + skip {B}x{s * h}x{s * w}x{Cs}, forward + backward: {CALLS_PER_GRAPH} calls per HIP-graph replay, "
           f"median of {rounds} alternating rounds of 10 replays",
           compare({"up_cat (one pass each way)": fused, "upsample_bilinear_ac + torch.cat": separate}, rounds), nbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-library", action="store_true", help="leave the F.conv2d side out of the depthwise comparison")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "deeplabv3plus_micro.py measures on the GPU"
    dev = torch.device("cuda:0")
    print(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}", flush=True)
    up_cat_micro(dev, args.rounds)
    depthwise_micro(dev, args.rounds, not args.skip_library)


if __name__ == "__main__":
    main()
