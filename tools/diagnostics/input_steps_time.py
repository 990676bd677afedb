"""Eager training step of AutoRegressiveLightning + HalfUNet at num_input_steps 1 and 2, native rollout and generic per-op path:
2 x 512 x 512, F = 60 state features (+ 5 forcings, 4 statics), T = 3 AR steps, bf16 matrix cores and bf16 storage.  Prints ONE
JSON line {"T_in=1/native": ms, ...}; "native_taken" reports whether common_step actually took the one-node native rollout
(otherwise the "native" time is the generic path's).

    python tools/diagnostics/input_steps_time.py [--steps 10] [--warmup 3] [--grid 512 512]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--pred-steps", type=int, default=3)
    args = ap.parse_args()

    from helpers import make_batch, make_dataset_info, synthetic_case
    from py4cast_amd.lightning import AutoRegressiveLightning

    dev = torch.device("cuda:0")
    H, W = args.grid
    B, T, F, Ff, Fs = args.batch, args.pred_steps, 60, 5, 4
    out = {"grid": [B, H, W, F], "T": T}
    for T_in in (1, 2):
        case = synthetic_case(seed=1, B=B, T=T, T_in=T_in, H=H, W=W, F=F, Ff=Ff, Fs=Fs)
        info = make_dataset_info(case, Ff)
        torch.manual_seed(0)
        lm = AutoRegressiveLightning(
            {"compute_dtype": "bf16", "activation_dtype": "bf16"}, info, None, num_input_steps=T_in, num_pred_steps_train=T,
            batch_size=B, model_name="HalfUNet",
            losses=[{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}],
            training_strategy="scaled_ar",
        ).to(dev)
        lm.train()
        batch = make_batch(case, dev)
        for route, native in (("native", True), ("generic", False)):
            lm.use_native_rollout = native
            if native:   # (with the generic path's fused step off, only the native rollout attaches a fused loss)
                lm.use_fused_step = False
                pred, _ = lm.common_step(batch, 0, "train")
                out[f"T_in={T_in}/native_taken"] = getattr(pred, "fused_loss", None) is not None
            lm.use_fused_step = True
            for i in range(args.warmup + args.steps):
                if i == args.warmup:
                    torch.cuda.synchronize()
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record()
                for p in lm.parameters():
                    p.grad = None
                lm.training_step(batch, 0).backward()
            t1.record()
            torch.cuda.synchronize()
            out[f"T_in={T_in}/{route}"] = t0.elapsed_time(t1) / args.steps
        del lm, batch
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
