import sys, torch
sys.path.insert(0, '/root/repo')
from py4cast_amd import ops
dev = torch.device('cuda:0')
B, T, H, W, F = 2, 3, 512, 512, 60
def t(fn, n=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3): fn()
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1000
x = torch.randn(B, T, H, W, F, device=dev); y = torch.randn(B, T, H, W, F, device=dev)
std = torch.rand(F, device=dev) + 0.5; mean = torch.randn(F, device=dev)
raw = torch.randn(F, B, T + 1, H, W, device=dev)
nb = x.numel() * 4
us = t(lambda: ops.unnormalize(x, std, mean, out=x)); print("unnormalize (B,T,512,512,60): %.1f us, %.2f TB/s" % (us, 2 * nb / us / 1e6))
us = t(lambda: ops.acc_sums(x, y, ops.MaskSpec(0), mean)); print("acc_sums: %.1f us, %.2f TB/s" % (us, 2 * nb / us / 1e6))
# one time step of prediction and target (2 x 512^2 x 60 each): the bytes p4c_psd reads; against 8 TB/s
us = t(lambda: ops.psd(x, y, ops.MaskSpec(0), T - 1)); print("psd (one step of B,512,512,60 x 2 tensors): %.1f us, %.2f TB/s, %.1f%% of 8 TB/s" % (us, 2 * nb / T / us / 1e6, 100 * 2 * nb / T / us / 1e6 / 8))
us = t(lambda: ops.pack_standardize(raw, mean, std)); print("pack_standardize (60 planes x B x 4 steps): %.1f us, %.2f TB/s" % (us, 2 * raw.numel() * 4 / us / 1e6))
