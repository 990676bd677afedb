"""UNet glue micro-timings: the encoder block tail at 2x512^2x64 bf16 against batch_norm_act + torch.cat + F.max_pool2d,
and the sub-pixel transposed-convolution GEMM against linear + interleave copy + torch.cat at the four UNet shapes.
usage: python tools/diagnostics/unet_micro.py  (one GPU, from the repository root)"""
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from py4cast_amd import ops_gemm as G
from py4cast_amd.unet import enc_tail, upconv_into
dev = torch.device("cuda:0")
def t(fn, n=20):
    for _ in range(3): fn()
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    torch.cuda.synchronize(); a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize(); return a.elapsed_time(b) / n * 1e3
B, H, W, C = 2, 512, 512, 64
y = torch.randn(B, H, W, C, device=dev).to(torch.bfloat16)
bn = torch.nn.BatchNorm2d(C).to(dev)
with torch.no_grad():
    us = t(lambda: enc_tail(y, None, bn.eval()))
    nbytes = 2 * (2 * y.numel() + y.numel() // 4)
    print(f"enc_tail fwd 2x512^2x64 bf16 (eval, no reduce): {us:.1f} us, {nbytes / us / 1e3:.0f} GB/s = {nbytes / us / 1e3 / 8000:.2f} of 8 TB/s")
    up = torch.randn(B, H, W, C, device=dev).to(torch.bfloat16)
    lib = lambda: F.max_pool2d(torch.cat((up, G.batch_norm_act(y, None, bn, slope=0.0)), -1)[..., C:].permute(0, 3, 1, 2), 2)
    print(f"library route batch_norm_act + cat + max_pool2d: {t(lib):.1f} us")
for Cin, Cout, h in ((1024, 512, 32), (512, 256, 64), (256, 128, 128), (128, 64, 256)):
    x = torch.randn(B, h, h, Cin, device=dev).to(torch.bfloat16)
    w = torch.randn(Cin, Cout, 2, 2, device=dev) / Cin ** 0.5
    b = torch.zeros(Cout, device=dev)
    buf = torch.empty(B, 2 * h, 2 * h, 2 * Cout, device=dev, dtype=torch.bfloat16)
    skip = torch.randn(B, 2 * h, 2 * h, Cout, device=dev).to(torch.bfloat16)
    with torch.no_grad():
        ours = t(lambda: upconv_into(x, w, b, buf))
        wr = w.permute(2, 3, 1, 0).reshape(4 * Cout, Cin)
        def lib():
            u = G.linear(x, wr).view(B, h, h, 2, 2, Cout).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * h, Cout)
            return torch.cat((u, skip), -1)
        print(f"upconv {Cin}->{Cout} at {h}x{h}: sub-pixel GEMM {ours:.1f} us, linear + interleave + cat {t(lib):.1f} us")
