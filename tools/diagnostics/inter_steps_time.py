"""Eager AutoRegressiveLightning + HalfUNet at 2 x 512 x 512, F = 60 state features (+ 5 forcings, 4 statics), bf16 matrix cores and
bf16 storage, for the two cases the native rollout covers beyond one model call per target step:

  * "train_K2_T3": a training step (rollout + loss + BPTT) with num_inter_steps = 2, T = 3, scaled_ar: 6 model calls;
  * "infer_T8":    a forecast (phase "inference", no_grad, eval) of T = 8 lead times, num_inter_steps = 1: 8 model calls.

Each case is timed on the native route and with ``use_native_rollout = False`` (the generic per-op path), the two alternating,
``--repeats`` times in one process.  Prints ONE JSON line: ms per MODEL CALL of every repeat, and "native_taken" -- whether the native
route really ran (no p4c_ar_update_fwd launch in one step); on a tree without the route both columns time the generic path.

    python tools/diagnostics/inter_steps_time.py [--steps 10] [--warmup 3] [--repeats 3] [--grid 512 512]
"""
import argparse
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def launches(fn):
    from py4cast_amd import _lib as L

    counts, real = collections.Counter(), L.call

    def counting(name, *a, **k):
        counts[name] += 1
        return real(name, *a, **k)

    L.call = counting
    try:
        fn()
    finally:
        L.call = real
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--grid", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--batch", type=int, default=2)
    args = ap.parse_args()

    from helpers import GRID_DIMS, feature_names, make_batch, make_dataset_info, synthetic_case
    from py4cast_amd.base import ItemBatch
    from py4cast_amd.lightning import AutoRegressiveLightning
    from py4cast_amd.namedtensor import NamedTensor

    dev = torch.device("cuda:0")
    H, W = args.grid
    B, F, Ff, Fs = args.batch, 60, 5, 4
    out = {"grid": [B, H, W, F], "unit": "ms per model call", "steps": args.steps, "warmup": args.warmup}
    for name, T, K in (("train_K2_T3", 3, 2), ("infer_T8", 8, 1)):
        case = synthetic_case(seed=1, B=B, T=T, T_in=1, H=H, W=W, F=F, Ff=Ff, Fs=Fs, border=2)
        info = make_dataset_info(case, Ff)
        torch.manual_seed(0)
        lm = AutoRegressiveLightning(
            {"compute_dtype": "bf16", "activation_dtype": "bf16"}, info, None, num_input_steps=1, num_pred_steps_train=T,
            batch_size=B, model_name="HalfUNet", num_inter_steps=K,
            losses=[{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}],
            training_strategy="scaled_ar",
        ).to(dev)
        batch = make_batch(case, dev)
        if name.startswith("train"):
            lm.train()

            def step():
                for p in lm.parameters():
                    p.grad = None
                lm.training_step(batch, 0).backward()
        else:
            lm.train()
            with torch.no_grad():
                lm.common_step(batch, 0, "val")   # records the feature names the forecast's result carries
            lm.eval()
            fbatch = ItemBatch(NamedTensor(case["inputs"].to(dev), GRID_DIMS, feature_names(F)),
                               NamedTensor(case["forcing"].to(dev), GRID_DIMS, [f"g{i}" for i in range(Ff)]), None)

            def step():
                with torch.no_grad():
                    lm.common_step(fbatch, 1, "inference")
        lm.use_native_rollout = True
        out[f"{name}/native_taken"] = launches(step)["p4c_ar_update_fwd"] == 0
        res = {"native": [], "generic": []}
        for _ in range(args.repeats):
            for route, native in (("native", True), ("generic", False)):
                lm.use_native_rollout = native
                res[route].append(round(timed(step, args.warmup, args.steps) / (T * K), 4))
        out[f"{name}/native"], out[f"{name}/generic"] = res["native"], res["generic"]
        del lm, batch
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
