"""Interleaved micro-benchmark of the latency-oriented 3x3 conv (csrc/conv_small.hip) against the kernel p4c_conv_fwd runs at the same
shape (row-streaming or ring kernel), in ONE process: per shape and forward mode (plain, plain + statistics, transform + statistics)
both kernels are checked against each other (stored map bit-equal, statistics relative) and then timed ALTERNATELY -- a captured graph
of N back-to-back launches of each, replayed in turn, so that neither the host's launch cost nor a clock drift favours one of them.
The last column is the small kernel with the in-kernel BatchNorm finalize (what the plan launches): its difference to the
statistics-only time is the finalize tail.  Output: profiles/small_conv_micro.txt.

    python tools/diagnostics/small_conv_micro.py [BxHxW ...]
"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from py4cast_amd import _lib as L, ops_model as om

dev = torch.device("cuda:0")
N, ROUNDS = 20, 7
shapes = sys.argv[1:] or ["2x256x256", "2x128x128", "2x64x64", "2x32x32", "2x256x320", "2x128x160", "2x64x80", "2x32x40"]


def graph_of(fn):
    fn(); fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(N):
            fn()
    return g


def timed(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); g.replay(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / N * 1000


for shp in shapes:
    B, H, W = (int(v) for v in shp.split("x"))
    torch.manual_seed(0)
    x = torch.randn(B, H, W, 64, device=dev).bfloat16()
    w = torch.randn(64, 64, 3, 3, device=dev) * 0.05
    sc = torch.rand(B, 64, device=dev) + 0.5
    sh = torch.randn(B, 64, device=dev) * 0.1
    gamma, beta = torch.rand(64, device=dev) + 0.5, torch.randn(64, device=dev)
    wp = om.prep_weights(w, False, 64, 64, compute="bf16")
    kind = {2: "rows", 1: "ring"}.get(L.lib().p4c_conv_kernel_kind(L.BF16, L.BF16, 64, 3, B, H, W), "tiled")
    routed = om.conv_small_ok(B, H, W)
    out_o, out_s = torch.empty_like(x), torch.empty_like(x)
    st_o = torch.empty(om.conv_tiles(B, H, W, 64, "bf16", storage=L.BF16), 2, 64, device=dev)
    st_s = torch.empty(B * L.lib().p4c_conv_small_stat_slots(B, H, W), 2, 64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    fin = [torch.empty(B, 64, device=dev) for _ in range(4)]

    def old(scale, shift, stats):
        L.call("p4c_conv_fwd", L.ptr(x), L.BF16, L.BF16, 64, L.ptr(wp), 3, L.ptr(scale), L.ptr(shift), int(scale is not None), None,
               L.ptr(out_o), 64, L.ptr(stats), B, H, W, 1, L.stream(dev))

    def new(scale, shift, stats, finalize=False, pre=None, src=None, dst=None):
        tail = [L.ptr(ticket), L.ptr(gamma), L.ptr(beta), 1e-5, 0.1, None, None] + [L.ptr(t) for t in fin] if finalize else \
               [None, None, None, 1e-5, 0.1, None, None, None, None, None, None]
        ptail = [L.ptr(pre), L.ptr(gamma), L.ptr(beta), None, None] + [L.ptr(t) for t in fin1] if pre is not None else [None] * 9
        L.call("p4c_conv_small_fwd", L.ptr(x if src is None else src), L.BF16, L.BF16, 64, L.ptr(wp), 3, L.ptr(scale), L.ptr(shift),
               int(scale is not None or pre is not None), None, L.ptr(out_s if dst is None else dst), 64, L.ptr(stats), B, H, W, 1,
               L.stream(dev), None, None, None, None, None, None, None, None, *tail, *ptail)

    fin1 = [torch.empty(B, 64, device=dev) for _ in range(4)]
    st_1, y1 = torch.empty_like(st_s), torch.empty_like(x)
    modes = {"plain": (None, None, None, None), "stats": (None, None, st_o, st_s), "transform+stats": (sc, sh, st_o, st_s)}
    for name, (a, b, so, ss) in modes.items():
        old(a, b, so); new(a, b, ss)
        torch.cuda.synchronize()
        line = "%-12s %-16s max |small - %s| = %g" % (shp, name, kind, (out_s.float() - out_o.float()).abs().max().item())
        if so is not None:
            t_o = so.view(B, -1, 2, 64).double().sum((0, 1)); t_s = ss.view(B, -1, 2, 64).double().sum((0, 1))
            line += ", statistics rel %.3g" % ((t_s - t_o).abs().max() / t_o.abs().max()).item()
        print(line, flush=True)
    for name, (a, b, so, ss) in modes.items():
        go, gs = graph_of(lambda: old(a, b, so)), graph_of(lambda: new(a, b, ss))
        gf = graph_of(lambda: new(a, b, ss, True)) if ss is not None else None
        to, ts, tf = [], [], []
        for _ in range(ROUNDS):
            to.append(timed(go)); ts.append(timed(gs))
            if gf is not None:
                tf.append(timed(gf))
        fmt = lambda t: "%.1f us (min %.1f)" % (sorted(t)[len(t) // 2], min(t))
        print("%-12s %-16s %s %s   small %s%s   [%s]" % (shp, name, kind, fmt(to), fmt(ts), "   small+finalize " + fmt(tf) if tf else "",
                                                          "routed" if routed else "not routed"), flush=True)
    if B * L.lib().p4c_conv_small_stat_slots(B, H, W) <= 256:
        # the two convolutions of a level, both with the in-kernel finalize as the plan launches them -- against the hand-off: the first
        # leaves its slots, the second finishes them in its prologue
        def pair_fin():
            new(None, None, st_1, True, dst=y1)
            new(fin[0], fin[1], st_s, True, src=y1)

        def pair_hand():
            new(None, None, st_1, False, dst=y1)
            new(None, None, st_s, True, pre=st_1, src=y1)

        gp, gh = graph_of(pair_fin), graph_of(pair_hand)
        tp, th = [], []
        for _ in range(ROUNDS):
            tp.append(timed(gp)); th.append(timed(gh))
        print("%-12s %-16s small, finalize in both %s   hand-off %s" % (shp, "level pair", fmt(tp), fmt(th)), flush=True)
