"""Eager AutoRegressiveLightning + HalfUNet (bf16 matrix cores, bf16 storage, scaled_ar, ``autopad_enabled``) on grids the network has to
pad, for the two cases the native rollout covers there (one input state, one model call per target step):

  * "train_T3": a training step (rollout + loss + BPTT) of T = 3 target steps: 3 model calls;
  * "infer_T8": a forecast (phase "inference", no_grad, eval) of T = 8 lead times: 8 model calls.

Shapes: 2 x 500 x 500 x 60 (+ 5 forcings, 4 statics; pads to 512 x 512) and the Titan-like 2 x 500 x 630 x 21 (+ 21 forcings; pads to
512 x 640), and -- as the ceiling -- the enclosing grids that fit, 2 x 512 x 512 x 60 and 2 x 512 x 640 x 21, where the native route has
its fused next input, fused 1x1 tail and saved loss gradients.

Each case is timed on the native route and with ``use_native_rollout = False`` (the generic per-op path: forward pads and crops around
the plan), the two alternating, ``--repeats`` times in one process.  Prints ONE JSON line: ms per MODEL CALL of every repeat, and
"native_taken" -- whether the native route really ran; on a tree without the padded route both columns of a padded shape time the
generic path.

    python tools/diagnostics/padded_rollout_time.py [--steps 10] [--warmup 3] [--repeats 3] [--entry-points]
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

SHAPES = (("500x500x60", 500, 500, 60, 5), ("500x630x21", 500, 630, 21, 21), ("512x512x60", 512, 512, 60, 5), ("512x640x21", 512, 640, 21, 21))


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
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--entry-points", action="store_true", help="also: [calls per step, mean us per call] of the native route's entry points")
    args = ap.parse_args()

    from helpers import GRID_DIMS, feature_names, make_batch, make_dataset_info, synthetic_case
    from py4cast_amd.base import ItemBatch
    from py4cast_amd.lightning import AutoRegressiveLightning
    from py4cast_amd.namedtensor import NamedTensor

    dev = torch.device("cuda:0")
    B, Fs = args.batch, 4
    out = {"unit": "ms per model call", "steps": args.steps, "warmup": args.warmup, "batch": B}
    for shape, H, W, F, Ff in SHAPES:
        for name, T in (("train_T3", 3), ("infer_T8", 8)):
            case = synthetic_case(seed=1, B=B, T=T, T_in=1, H=H, W=W, F=F, Ff=Ff, Fs=Fs, border=2)
            info = make_dataset_info(case, Ff)
            torch.manual_seed(0)
            lm = AutoRegressiveLightning(
                {"compute_dtype": "bf16", "activation_dtype": "bf16", "autopad_enabled": True}, info, None, num_input_steps=1,
                num_pred_steps_train=T, batch_size=B, model_name="HalfUNet", num_inter_steps=1,
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
            n = launches(step)
            # the generic route updates the state with p4c_ar_update_fwd (forecast) and differentiates build_x per call (training)
            out[f"{shape}/{name}/native_taken"] = n["p4c_ar_update_fwd"] == 0 and n["p4c_build_x_bwd"] == 0
            res = {"native": [], "generic": []}
            for _ in range(args.repeats):
                for route, native in (("native", True), ("generic", False)):
                    lm.use_native_rollout = native
                    res[route].append(round(timed(step, args.warmup, args.steps) / T, 4))
            out[f"{shape}/{name}/native"], out[f"{shape}/{name}/generic"] = res["native"], res["generic"]
            if args.entry_points:
                # where the native route's time goes: a HIP event pair around every call of the model's entry points (a run of its
                # own; the weight gradients of the backward plan run on a side stream beside what these pairs bracket)
                from py4cast_amd import _lib as L

                lm.use_native_rollout = True
                L.enable_kernel_timing(lm.model.timed_entry_points)
                for _ in range(3):
                    step()
                out[f"{shape}/{name}/entry_points_us"] = {k: [c // 3, round(1e3 * ms, 1)] for k, (c, ms) in sorted(L.kernel_times().items())}
                L.enable_kernel_timing(None)
            del lm, batch
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
