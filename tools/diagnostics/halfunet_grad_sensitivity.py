"""Sensitivity of the HalfUNet parameter gradients to a tiny perturbation of the first convolution's output, in float64 on the CPU (no
GPU): the oracle network (oracle/halfunet.py) with the draws of tests/test_wide_input_gpu.py::test_wide_halfunet_plan_matches_oracle,
run once plain and once with the first convolution's output multiplied by (1 + eps * noise).  ReLU / max-pool decisions within eps of
a tie flip, and the largest relative change of any parameter gradient is what any two fp32 implementations of the network may
differ by -- the floor that test's bars are derived from.  Prints one JSON line per case.

    python tools/diagnostics/halfunet_grad_sensitivity.py [--eps 1e-6]
"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

CASES = [("batch", 129, 60, 64, 64), ("batch", 189, 60, 32, 48), ("group", 100, 21, 48, 32), ("batch", 89, 40, 32, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eps", type=float, default=1e-6)
    args = ap.parse_args()
    from oracle.halfunet import HalfUNetRef

    for norm, cin, cout, H, W in CASES:
        torch.manual_seed(0)   # as tests/test_wide_input_gpu.py::_make_pair
        ref = HalfUNetRef(cin, cout, norm=norm)
        with torch.no_grad():
            for m in ref.modules():
                if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.GroupNorm)):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-0.3, 0.3)
        g = torch.Generator().manual_seed(3)
        x = torch.randn(2, H, W, cin, generator=g)
        gy = torch.randn(2, H, W, cout, generator=g)

        def grads(eps):
            r = copy.deepcopy(ref).double().train()
            if eps:
                noise = torch.Generator().manual_seed(1)
                r.encoder1.enc1conv1.register_forward_hook(
                    lambda m, i, o: o * (1 + eps * torch.randn(o.shape, generator=noise, dtype=o.dtype)))
            y = r(x.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
            (y * gy.double()).sum().backward()
            return {n: p.grad for n, p in r.named_parameters()}

        a, b = grads(0.0), grads(args.eps)
        rel = {n: float((b[n] - a[n]).abs().max() / a[n].abs().max()) for n in a}
        worst = max(rel, key=rel.get)
        print(json.dumps({"norm": norm, "cin": cin, "cout": cout, "grid": [H, W], "eps": args.eps, "max_rel_change": rel[worst],
                          "parameter": worst}))


if __name__ == "__main__":
    main()
