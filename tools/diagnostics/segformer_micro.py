"""Segformer step micro-timing: one training step -- a 3-step autoregressive chain of the model at 2 x 512^2 with 60
predicted fields (69 input channels: the previous prediction + 9 constant forcing / static channels), MSE loss, backward -- of
  native : SegformerMI355X on the bf16 route (eager launches, no HIP graph), and
  library: the float restatement (tests/segformer_reference.py, fp32 parameters) under torch.autocast(bfloat16),
alternated in the same process, REPEATS rounds of STEPS steps each; prints the per-round ms / step of both and their medians / spreads.
usage: python tools/diagnostics/segformer_micro.py  (one GPU, from the repository root)"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from py4cast_amd.segformer import SegformerMI355X, SegformerSettings  # noqa: E402
from segformer_reference import SegformerReference  # noqa: E402

B, H, W, FO, EXTRA, T = 2, 512, 512, 60, 9, 3
STEPS, REPEATS = 10, 5
dev = torch.device("cuda:0")
torch.manual_seed(0)
native = SegformerMI355X(FO + EXTRA, FO, (H, W), SegformerSettings(compute_dtype="bf16")).to(dev)
ref = SegformerReference(FO + EXTRA, FO).to(dev)
ref.load_state_dict(native.state_dict())
x0 = torch.randn(B, H, W, FO, device=dev)
const = torch.randn(B, H, W, EXTRA, device=dev)
target = torch.randn(B, H, W, FO, device=dev)


def step_native():
    native.zero_grad(set_to_none=True)
    s, c = x0.to(torch.bfloat16), const.to(torch.bfloat16)
    loss = 0.0
    for _ in range(T):
        s = native(torch.cat((s, c, torch.zeros_like(c[..., :72 - FO - EXTRA])), -1)).to(torch.bfloat16)
        loss = loss + F.mse_loss(s.float(), target)
    loss.backward()


def step_library():
    ref.zero_grad(set_to_none=True)
    s, c = x0.permute(0, 3, 1, 2), const.permute(0, 3, 1, 2)
    loss = 0.0
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for _ in range(T):
            s = ref(torch.cat((s, c.to(s.dtype)), 1))
            loss = loss + F.mse_loss(s.float(), target.permute(0, 3, 1, 2))
    loss.backward()


def timed(fn):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(STEPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / STEPS


for _ in range(3):
    step_native()
    step_library()
res = {"native": [], "library": []}
for r in range(REPEATS):
    res["native"].append(timed(step_native))
    res["library"].append(timed(step_library))
    print(f"round {r}: native bf16 {res['native'][-1]:.2f} ms/step, autocast restatement {res['library'][-1]:.2f} ms/step", flush=True)
for k, v in res.items():
    print(f"{k}: median {statistics.median(v):.2f} ms/step, min {min(v):.2f}, max {max(v):.2f} (over {REPEATS} rounds of {STEPS} steps)")
print(f"speed-up (medians): {statistics.median(res['library']) / statistics.median(res['native']):.2f}x")
