import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
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


# ---- the observers' fused evaluation pass (ops.eval_sums) against the sequence it replaces, same run, alternating, HIP events:
# masked_count (with a mask only) + scaled_loss(L1) + scaled_loss(MSE) + weighted_loss_map.  Rates against ALGORITHMIC bytes:
# fused = prediction + target once (+ the (T,N) map); replaced = one array per masked_count, two per loss call, + the (B,T,N) map.
def eval_observers(out_path):
    import os
    from py4cast_amd import _lib as L
    lines = []
    for shape in ((2, 3, 512, 512, 60), (2, 3, 512, 640, 21)):
        B, T, H, W, F = shape
        N = H * W
        p = torch.randn(shape, device=dev); g = torch.randn(shape, device=dev)
        g_nan = g.clone(); g_nan[torch.rand(shape, device=dev) < 0.01] = float("nan")
        std = torch.rand(F, device=dev) + 0.5; w = torch.rand(F, device=dev) + 0.5
        interior = torch.ones(N, device=dev); amap = torch.zeros(T, H, W, device=dev)
        nb = p.numel() * 4
        for label, spec, tgt in (("no mask", ops.MaskSpec(L.MASK_NONE), g), ("mask from NaN", ops.MaskSpec(L.MASK_FROM_NAN), g_nan)):
            def fused():
                ops.eval_sums(p, tgt, spec, std, interior, float(N), w, L.LOSS_MSE, amap, True)
            def replaced():
                c = ops.masked_count(spec, tgt)
                ops.scaled_loss(p, tgt, spec, std, interior, float(N), L.LOSS_L1, count=c)
                ops.scaled_loss(p, tgt, spec, std, interior, float(N), L.LOSS_MSE, count=c)
                ops.weighted_loss_map(p, tgt, spec, w, L.LOSS_MSE)
            tf, tr = [], []
            for _ in range(5):   # alternate: both see the same neighbours on a shared machine
                tf.append(t(fused)); tr.append(t(replaced))
            uf, ur = sorted(tf)[2], sorted(tr)[2]
            bytes_f = 2 * nb + T * N * 4 * 2
            bytes_r = (1 if spec.mode else 0) * nb + 6 * nb + B * T * N * 4
            lines.append("%s, %s: fused %.1f us (%.2f TB/s; runs %s) | replaced %.1f us (%.2f TB/s; runs %s) | ratio %.2f" % (
                "x".join(map(str, shape)), label, uf, bytes_f / uf / 1e6, " ".join("%.0f" % v for v in tf), ur, bytes_r / ur / 1e6,
                " ".join("%.0f" % v for v in tr), ur / uf))
    text = "ops.eval_sums against masked_count + 2 x scaled_loss + weighted_loss_map (median of 5 alternating rounds of 20 calls)\n" + "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write(text)


eval_observers(os.path.join(ROOT, "profiles", "eval_observers.txt"))
