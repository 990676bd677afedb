"""CustomUNet against the library on the GPU (profiles/customunet_vs_library.txt):

1. up2cat (csrc/customunet.hip: nearest x2 + skip concatenation, forward + backward) against F.interpolate + torch.cat and their autograd
   backward, at the four concatenating decoder geometries of the bench shape (2 x 512 x 512).  A call is ~10 us of kernel time behind
   ~50 us of host work, so each side's 20 forward + backward calls are captured into one HIP graph (one stream) and the replays are
   timed with device events: median of 5 alternating rounds of 10 replays; achieved rate = the algorithmic bytes of the FUSED pair
   (forward x + skip + out, backward dout + dx + dskip) over the time, against 8 TB/s.
2. the bench step (bench.py --model CustomUNet --strategy diff_ar: 2 x 512 x 512 x 60, T = 3; rollout + loss + backward + AdamW) on the
   native bf16 route against the same step with the restatement (tests/customunet_reference.py) under bf16 autocast on library kernels:
   same process, same batch, median of 5 alternating rounds of 5 steps.

    python tools/diagnostics/customunet_micro.py [--rounds 5] [--grid 512 512]
"""
import argparse
import os
import statistics
import sys
from dataclasses import dataclass

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = 8e12


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def alternating(f_new, f_old, rounds, n):
    for f in (f_new, f_old):
        timed(f, 3)
    new, old = [], []
    for _ in range(rounds):
        new.append(timed(f_new, n))
        old.append(timed(f_old, n))
    return new, old


CALLS_PER_GRAPH = 20


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


def up2cat_micro(dev, rounds, H, W):
    from py4cast_amd.customunet import up2_cat

    print(f"up2cat forward + backward against interpolate + cat (+ their autograd backward), batch 2, grid {H}x{W}: {CALLS_PER_GRAPH} calls "
          f"per HIP-graph replay, median of {rounds} alternating rounds of 10 replays, time per call")
    g = torch.Generator(device=dev).manual_seed(0)
    for blk, (stride, Cx, Cs) in enumerate(((32, 512, 256), (16, 256, 128), (8, 128, 64), (4, 64, 64))):
        h, w = H // stride, W // stride
        x = torch.randn(2, h, w, Cx, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
        skip = torch.randn(2, 2 * h, 2 * w, Cs, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
        dout = torch.randn(2, 2 * h, 2 * w, Cx + Cs, device=dev, generator=g).to(torch.bfloat16)
        dout_nchw = dout.permute(0, 3, 1, 2)       # (the same memory: channels-last)

        def fused():
            x.grad = skip.grad = None
            up2_cat(x, skip).backward(dout)

        def library():
            x.grad = skip.grad = None
            up = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
            torch.cat([up, skip.permute(0, 3, 1, 2)], dim=1).backward(dout_nchw)

        fused()
        gx, gs = x.grad.clone(), skip.grad.clone()
        library()
        assert torch.equal(gs, skip.grad) and float((gx.float() - x.grad.float()).abs().max()) <= 2.0 ** -6 * float(gx.float().abs().max())
        new, old = alternating(captured(fused), captured(library), rounds, 10)
        new, old = [t / CALLS_PER_GRAPH for t in new], [t / CALLS_PER_GRAPH for t in old]
        tn, to = statistics.median(new), statistics.median(old)
        nbytes = 2 * 2 * (x.numel() + skip.numel() + dout.numel())
        us = lambda v: " ".join(f"{1e6 * t:.1f}" for t in v)      # noqa: E731
        print(f"block {blk}: x 2x{h}x{w}x{Cx} + skip {Cs}: fused {1e6 * tn:.1f} us ({nbytes / tn / 1e12:.2f} TB/s = "
              f"{100 * nbytes / tn / PEAK:.1f} % of 8 TB/s; runs {us(new)}) | interpolate + cat {1e6 * to:.1f} us "
              f"({nbytes / to / 1e12:.2f} TB/s on the same byte count; runs {us(old)}) | ratio {to / tn:.2f}")


@dataclass
class _LibrarySettings:
    encoder_name: str = "resnet18"


def _library_model_class():
    from customunet_reference import CustomUNetReference
    from py4cast_amd.base import ModelABC, ModelType

    class CustomUNetLibrary(ModelABC, torch.nn.Module):
        """the restatement under bf16 autocast: every convolution, norm, pool, interpolate and cat on library kernels"""

        settings_kls = _LibrarySettings
        onnx_supported = False
        supported_num_spatial_dims = (2,)
        num_spatial_dims = 2
        features_last = True
        model_type = ModelType.CONVOLUTIONAL
        register = True

        def __init__(self, in_channels, out_channels, input_shape, settings=None, *args, **kwargs):
            super().__init__()
            self.in_channels, self.out_channels, self.input_shape = in_channels, out_channels, input_shape
            self._settings = settings
            self.net = CustomUNetReference(in_channels, out_channels, settings.encoder_name)
            self.check_required_attributes()

        @property
        def settings(self):
            return self._settings

        def forward(self, x):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = self.net(x)
            return y.to(x.dtype)

    return CustomUNetLibrary


def step_compare(dev, rounds, H, W):
    import bench
    from py4cast_amd.lightning import AutoRegressiveLightning
    from py4cast_amd.models import registry
    from py4cast_amd.trainer import FlatDDP

    registry.setdefault("CustomUNetLibrary", _library_model_class())
    B, Fe, T, Ff, Fs = 2, 60, 3, 5, 4
    case = bench.synthetic_case(1234, B, T, 1, H, W, Fe, Ff, Fs, 0, dev)
    info = bench.make_info(case, Ff)

    def build(name, settings):
        torch.manual_seed(1234)
        lm = AutoRegressiveLightning(settings, info, None, num_input_steps=1, num_pred_steps_train=T, num_pred_steps_val_test=T, batch_size=B,
                                     model_name=name,
                                     losses=[{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}],
                                     training_strategy="diff_ar", learning_rate=1e-3, min_learning_rate=3e-7, num_warmup_steps=1000,
                                     betas=(0.9, 0.95)).to(dev)
        ddp = FlatDDP(lm.model, 1)
        opt = lm.configure_optimizers()["optimizer"]
        losses = []

        def step():
            loss = lm.training_step(bench.make_batch(case), 0)
            loss.backward()
            ddp.all_reduce_grads()
            opt.step()
            ddp.zero_grad()
            losses.append(loss.detach())

        return lm, step, losses

    lm_n, native, ln = build("CustomUNet", dict(bench.model_settings("CustomUNet", "bf16"), encoder_weights=False))
    lm_l, library, ll = build("CustomUNetLibrary", {})
    lm_l.model.net.load_state_dict(lm_n.model.state_dict())
    new, old = alternating(native, library, rounds, 5)
    tn, to = statistics.median(new), statistics.median(old)
    ms = lambda v: " ".join(f"{1e3 * t:.2f}" for t in v)      # noqa: E731
    print(f"bench step (CustomUNet resnet18, diff_ar, {B}x{H}x{W}x{Fe}, T = {T}; rollout + loss + backward + AdamW), median of {rounds} "
          f"alternating rounds of 5 steps")
    print(f"native bf16 {1e3 * tn:.2f} ms per step (runs {ms(new)}) | restatement under bf16 autocast on library kernels {1e3 * to:.2f} ms per "
          f"step (runs {ms(old)}) | ratio {to / tn:.2f}")
    print(f"first-step loss: native {float(ln[0]):.6f}, library {float(ll[0]):.6f} (equal initial weights, same batch)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--grid", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "customunet_micro.py measures on the GPU"
    dev = torch.device("cuda:0")
    H, W = args.grid
    up2cat_micro(dev, args.rounds, H, W)
    if not args.skip_step:
        step_compare(dev, args.rounds, H, W)


if __name__ == "__main__":
    main()
