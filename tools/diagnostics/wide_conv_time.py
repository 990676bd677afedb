"""Launches of the K-chunked first convolution (conv_fwd_bf16_wide, bf16 storage) at 2 x 512 x 512 for cin_pad 160 (129 real input
channels: num_input_steps = 2 at F = 60) and 256, with statistics, for a `rocprofv3 --kernel-trace --stats` run of its own.  Prints
the event-timed average per launch as one JSON line.

    python tools/diagnostics/wide_conv_time.py [--launches 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    from py4cast_amd import ops_model as om

    dev = torch.device("cuda:0")
    B, H, W = 2, 512, 512
    res = {}
    for CI, CIreal in ((160, 129), (256, 249)):
        x = torch.randn(B, H, W, CI, device=dev)
        x[..., CIreal:] = 0
        x = x.bfloat16()
        w = torch.randn(64, CIreal, 3, 3, device=dev) * 0.05
        wp = om.prep_weights(w, False, 64, CI, compute="bf16")
        for _ in range(3):
            om.conv_fwd(x, wp, 3, want_stats=True, compute="bf16")
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.launches):
            om.conv_fwd(x, wp, 3, want_stats=True, compute="bf16")
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.launches
        flops = 2.0 * 9 * CIreal * 64 * B * H * W
        res[f"cin_pad={CI}"] = {"cin": CIreal, "ms_per_launch_incl_alloc": ms, "real_tflops": flops / (ms * 1e-3) / 1e12}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
