"""The first convolution 69 -> 64 at the benchmark shape (2 x 512 x 512, 96-channel pixels) through the single-op entry points, the
one-launch row kernel (p4c_first_conv_one) against row launch + tail (p4c_first_conv_two), alternating in one process: blocks of 20
calls between two HIP events, 7 rounds, the first discarded.  Every call of either form also runs the weight-preparation launch of the
entry point (one small kernel, the same for both) and a stream-ordered allocation, so the per-call figure is an upper bound of the
kernels' own time; the DIFFERENCE of the two forms is what the plan saves per model call.
usage: python tools/diagnostics/first_conv_micro.py > profiles/first_conv_one_launch_micro.txt"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from py4cast_amd import _lib as L  # noqa: E402

dev = torch.device("cuda:0")
B, H, W, cin, x_cs, N = 2, 512, 512, 69, 96, 20
g = torch.Generator().manual_seed(0)
x = torch.zeros(B, H, W, x_cs)
x[..., :cin] = torch.randn(B, H, W, cin, generator=g)
x = x.bfloat16().to(dev)
w = (torch.randn(64, cin, 3, 3, generator=g) * 0.2).to(dev)
y = torch.empty(B, H, W, 64, dtype=torch.bfloat16, device=dev)
lib = L.lib()
slots = max(lib.p4c_first_conv_one_slots(B, H, W), lib.p4c_first_conv_tail_slots(B, H, W))
st = torch.empty(B, slots, 2, 64, device=dev)


def block(name):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(N):
        L.call(name, L.ptr(x), x_cs, cin, L.ptr(w), L.ptr(y), L.ptr(st), B, H, W, L.stream(dev))
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / N


res = {"p4c_first_conv_one": [], "p4c_first_conv_two": []}
for r in range(7):
    for name in res:
        t = block(name)
        if r:
            res[name].append(t)
print(f"# first convolution {cin} -> 64 at {B} x {H} x {W}, {x_cs}-channel pixels, statistics on; us per call, blocks of {N} calls, alternating")
for name, v in res.items():
    print(f"{name}: " + " ".join(f"{t:.1f}" for t in v) + f"   median {statistics.median(v):.1f}")
d = statistics.median(res["p4c_first_conv_two"]) - statistics.median(res["p4c_first_conv_one"])
print(f"row launch + tail minus one launch: {d:.1f} us per call")
