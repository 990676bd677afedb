"""
The references and the launch mirror of tests/gnn_nodes.py themselves, without a GPU:

* the composed float64 references, run on a model's state dict, are oracle/graphlam.py, oracle/hilam.py's HiLam and HiLamParallel: output,
  dx and every parameter gradient to 1e-10, at 36 x 45 (81 mesh nodes, levels [81, 9]) and at 81 x 96 (levels [729, 81, 9]: the smallest grid
  where HiLAM's down / up sweeps have an interior level) -- in the concat formulation and in the distributed one the native models run;
* the distributed first Linear + gathered addends is the Linear over the concatenation; segment_sum is a Python loop, receivers without
  edges included; the mean aggregation divides by the in-degree;
* the launch mirror: slots, passes, splits and caps on both sides of every threshold, against values written out by hand from the launch
  code (csrc/mlp.hip mlp_grid / mlp_bwd_slots, csrc/graph.hip segment_sum_shape / launch_gather_add, csrc/nodeproj.hip proj_grid /
  wgrad_grid / wgrad_slots); the caps grid at 256 CUs is smaller than 512 x 512, has the benchmark's hierarchy and loop signature, row
  counts that are no multiple of 32, and a table that differs from the toy grid's.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gnn_nodes as N  # noqa: E402


def rel(got, ref):
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def unit_meshgrid(H, W):
    ys, xs = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    return torch.stack([xs, ys])


def flat_graph(H, W):
    from py4cast_amd.graph_build import build_mesh_graph

    g = build_mesh_graph(unit_meshgrid(H, W))
    d = {k: getattr(g, k) for k in ("g2m", "m2m", "m2g", "mesh_pos")}
    d.update({f"{k}_feat": getattr(g, f"{k}_feat") for k in ("g2m", "m2m", "m2g")})
    return d


def hi_graph(H, W):
    from py4cast_amd.graph_build import build_hierarchical_graph

    g = build_hierarchical_graph(unit_meshgrid(H, W))
    return {k: getattr(g, k) for k in ("g2m", "m2g", "g2m_feat", "m2g_feat", "mesh_pos", "same", "same_feat", "up", "up_feat", "down", "down_feat")}


def against_oracle(oracle, network, cin, cout, n_grid, seed):
    torch.manual_seed(seed)
    with torch.no_grad():
        for n, p in oracle.named_parameters():
            if n.endswith(("3.weight", "3.bias")):          # LayerNorm affine off 1 / 0
                p.add_(0.1 + 0.2 * torch.rand_like(p))
    x, dy = torch.randn(2, n_grid, cin, dtype=torch.float64), torch.randn(2, n_grid, cout, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    yr = oracle(xr)
    yr.backward(dy)
    for form in (N.interaction_net, N.interaction_net_distributed):
        P = {n: p.detach().clone().requires_grad_(True) for n, p in oracle.named_parameters()}
        xg = x.clone().requires_grad_(True)
        y = network(xg, P, form)
        y.backward(dy)
        assert rel(y.detach(), yr.detach()) <= 1e-10, form.__name__
        assert rel(xg.grad, xr.grad) <= 1e-10, form.__name__
        for n, p in oracle.named_parameters():
            assert P[n].grad is not None and rel(P[n].grad, p.grad) <= 1e-10, (form.__name__, n)


@pytest.mark.parametrize("H,W", [(36, 45), (81, 96)])
@pytest.mark.parametrize("aggr", ["sum", "mean"])
def test_graphlam_reference_is_the_oracle(H, W, aggr):
    from oracle.graphlam import GraphLam

    g = flat_graph(H, W)
    torch.manual_seed(3)
    oracle = GraphLam(13, 5, g, processor_layers=2, mesh_aggr=aggr).double()
    against_oracle(oracle, lambda x, P, form: N.graphlam_network(x, P, g, aggr, form), 13, 5, H * W, 4)


@pytest.mark.parametrize("H,W,levels", [(36, 45, [81, 9]), (81, 96, [729, 81, 9])])
@pytest.mark.parametrize("model", ["hilam", "hilampar"])
def test_hilam_references_are_the_oracles(H, W, levels, model):
    from oracle.hilam import HiLam, HiLamParallel

    g = hi_graph(H, W)
    assert [p.shape[0] for p in g["mesh_pos"]] == levels == N.mesh_levels(H, W)
    torch.manual_seed(5)
    oracle = (HiLam if model == "hilam" else HiLamParallel)(11, 4, g, processor_layers=2).double()
    net = N.hilam_network if model == "hilam" else N.hilampar_network
    # (HiLAMParallel's processor has one formulation, per edge set; its encoder / init / read-out InteractionNets take both)
    against_oracle(oracle, lambda x, P, form: net(x, P, g, form), 11, 4, H * W, 6)


def test_distributed_first_linear_is_the_concat_linear():
    torch.manual_seed(7)
    ns, nr, E = 37, 23, 301
    d = torch.float64
    e, s, r = torch.randn(E, 64, dtype=d), torch.randn(ns, 64, dtype=d), torch.randn(nr, 64, dtype=d)
    src, dst = torch.randint(0, ns, (E,)), torch.randint(0, nr, (E,))
    w, b = torch.randn(64, 192, dtype=d), torch.randn(64, dtype=d)
    concat = N.linear(torch.cat([e, s[src], r[dst]], dim=-1), w, b)
    pa, pb = N.node_proj(s, [w[:, 64:128]])[0], N.node_proj(r, [w[:, 128:]])[0]
    dist = N.edge_gather_add(N.linear(e, w[:, :64], b), pa, src, pb, dst)
    assert rel(dist, concat) <= 1e-13
    # and inside the fused MLP: the gathered addends enter before the SiLU
    w2, b2, g_, bt = torch.randn(64, 64, dtype=d), torch.randn(64, dtype=d), torch.rand(64, dtype=d) + 0.5, torch.randn(64, dtype=d)
    y, yr = N.row_mlp(e, w[:, :64], b, w2, b2, g_, bt, ga=pa, ia=src, gb=pb, ib=dst, res=e)
    want = torch.nn.functional.layer_norm(torch.nn.functional.silu(concat) @ w2.t() + b2, (64,), g_, bt)
    assert rel(y, want) <= 1e-13 and rel(yr, want + e) <= 1e-13
    # the passthrough tensor's gradient is summed into dx
    x = s.clone().requires_grad_(True)
    a, x_back = N.node_proj(x, [w[:, :64]], passthrough=True)
    da, dres = torch.randn_like(a), torch.randn_like(x)
    torch.autograd.backward([a, x_back], [da, dres])
    assert rel(x.grad, da @ w[:, :64] + dres) <= 1e-13


def test_row_mlp_reference_handles_narrow_shapes():
    """K below the padded width (the first w1.shape[1] features count), fewer than 64 outputs without LayerNorm, row-aligned addends"""
    torch.manual_seed(8)
    d = torch.float64
    x = torch.randn(50, 80, dtype=d)
    w1, b1, w2, b2 = torch.randn(64, 69, dtype=d), torch.randn(64, dtype=d), torch.randn(60, 64, dtype=d), torch.randn(60, dtype=d)
    ga = torch.randn(50, 64, dtype=d)
    y, yr = N.row_mlp(x, w1, b1, w2, b2, ga=ga)
    want = torch.nn.functional.silu(x[:, :69] @ w1.t() + b1 + ga) @ w2.t() + b2
    assert yr is None and y.shape == (50, 60) and rel(y, want) <= 1e-13
    h = torch.nn.functional.silu(x[:, :69] @ w1.t() + b1 + ga)
    yq, _ = N.row_mlp(x, w1, b1, w2, b2, ga=ga, round_hidden=True)
    assert rel(yq, h.to(torch.bfloat16).double() @ w2.t() + b2) <= 1e-13 and 1e-4 < rel(yq, y) < 1e-2


def test_segment_sum_is_a_python_loop():
    torch.manual_seed(9)
    n, E = 41, 500
    dst = torch.randint(0, n, (E,))
    dst[dst == 7] = 8
    dst[dst == 40] = 0                                   # receivers 7 and 40 (the last) have no edges
    msg = torch.randn(E, 64, dtype=torch.float64)
    want = torch.zeros(n, 64, dtype=torch.float64)
    for e in range(E):
        want[dst[e]] += msg[e]
    got = N.segment_sum(msg, dst, n)
    assert rel(got, want) <= 1e-14 and not got[7].any() and not got[40].any()
    # its adjoint is the gather
    m = msg.clone().requires_grad_(True)
    dy = torch.randn(n, 64, dtype=torch.float64)
    N.segment_sum(m, dst, n).backward(dy)
    assert torch.equal(m.grad, N.rows_of(dy, dst))
    # mean: the sum over the in-degree; a receiver without edges stays zero (no division by zero)
    deg = torch.tensor([int((dst == r).sum()) for r in range(n)])
    assert torch.equal(N.in_degree(dst, n), deg)
    mean = N.mean_of_sum(got, dst, n)
    for r in range(n):
        assert torch.allclose(mean[r], want[r] / max(int(deg[r]), 1), rtol=1e-14, atol=0)
    assert torch.isfinite(mean).all()


# ------------------------------------------------------------------------------------------------ the launch mirror, by hand
# row_mlp: 32-row tiles, 4 per workgroup (128 rows); forward cap 4 x CUs, backward cap CUs.  (R, cus) -> grid fwd, passes fwd, capped fwd,
# grid bwd, passes bwd, slots bwd, capped bwd
MLP_BY_HAND = [
    ((1, 256), (1, 1, False, 1, 1, 1, False)),                   # one tile: one wave, one slot
    ((100, 256), (1, 1, False, 1, 1, 4, False)),                 # 4 tiles in one workgroup: per-wave slots
    ((2048, 256), (16, 1, False, 16, 1, 64, False)),             # 16 workgroups = PER_WAVE_MAX_G: still per-wave slots (64)
    ((2049, 256), (17, 1, False, 17, 1, 17, False)),             # 17 workgroups: one slot per workgroup
    ((32768, 256), (256, 1, False, 256, 1, 256, False)),         # backward exactly at its cap
    ((32769, 256), (257, 1, False, 256, 2, 256, True)),          # one row more: 1025 tiles on 1024 waves, the backward loops
    ((131072, 256), (1024, 1, False, 256, 4, 256, True)),        # forward exactly at its cap
    ((131073, 256), (1024, 2, True, 256, 5, 256, True)),         # the forward loops
    ((65553, 256), (513, 1, False, 256, 3, 256, True)),          # 128 x 256 x 2 + 17
    ((131105, 256), (1024, 2, True, 256, 5, 256, True)),         # 512 x 256 + 33
    ((1000, 4), (8, 1, False, 4, 2, 16, True)),                  # 4 CUs: backward capped at 4 workgroups <= 16: per-wave slots min(32, 16)
    ((16385, 128), (129, 1, False, 128, 2, 128, True)),
]


@pytest.mark.parametrize("size,want", MLP_BY_HAND)
def test_mlp_launch_mirror(size, want):
    R, cus = size
    f, b = N.mlp_launch(R, 4, cus), N.mlp_launch(R, 1, cus, bwd=True)
    assert (N.mlp_grid(R, 4, cus), f.passes, f.capped, N.mlp_grid(R, 1, cus), b.passes, b.slots, b.capped) == want
    assert b.slots == N.mlp_bwd_slots(R, cus) and f.slots is None


# segment_sum over 64 bf16 features: 8 chunks, lpr_log2 3, 8 lane groups per wave; split from the mean list length (4 << split < mean);
# cap 16 x CUs workgroups of 4 waves.  (N, E, cus) -> blocks, split_log2, passes, capped
SEG_BY_HAND = [
    ((1000, 4000, 256), (32, 0, 1, False)),                      # mean 4: no split, 8 segments per wave, 125 waves
    ((1000, 4001, 256), (63, 1, 1, False)),                      # mean 5 > 4: split 2, 4 segments per wave, 250 waves
    ((1000, 8001, 256), (125, 2, 1, False)),                     # mean 9 > 8: split 4
    ((1000, 16001, 256), (250, 3, 1, False)),                    # mean 17 > 16: split 8, one segment per wave
    ((1000, 10 ** 6, 256), (250, 3, 1, False)),                  # the split stops at the wave's 8 groups
    ((131072, 131072, 256), (4096, 0, 1, False)),                # split 0 exactly at the cap: 16384 waves
    ((131073, 131073, 256), (4096, 0, 2, True)),                 # one more segment: a ninth of the waves takes a second pass
    ((16384, 16384 * 33, 256), (4096, 3, 1, False)),             # split 8 exactly at the cap
    ((16385, 16385 * 33, 256), (4096, 3, 2, True)),
    ((13122, 389764, 256), (3281, 3, 1, False)),                 # the g2m aggregation of 2 x 243 x 288: mean 30, below the cap
    ((100, 0, 256), (4, 0, 1, False)),                           # no edges at all
    ((1000, 4000, 2), (32, 0, 1, False)), ((1025, 4100, 2), (32, 0, 2, True)),
]


@pytest.mark.parametrize("size,want", SEG_BY_HAND)
def test_segment_sum_launch_mirror(size, want):
    n, E, cus = size
    blocks, lpr_log2, split_log2 = N.segment_sum_shape(n, E, 8, cus)
    l = N.segment_sum_launch(n, E, cus)
    assert lpr_log2 == 3 and (blocks, split_log2, l.passes, l.capped) == want and l.split_log2 == split_log2
    assert N.segment_sum_shape(n, E, 16, cus)[1] == 4 and N.segment_sum_shape(n, E, 200, cus)[1] == 6       # fp32 rows; the clamp at a wave


# edge_gather_add, 8 chunks: 8 rows per wave instruction, 16 per pass, 64 per workgroup, cap 16 x CUs.  (E, cus) -> blocks, passes, capped
GATHER_BY_HAND = [((1, 256), (1, 1, False)), ((64, 256), (1, 1, False)), ((65, 256), (2, 1, False)), ((262144, 256), (4096, 1, False)),
                  ((262145, 256), (4096, 2, True)), ((10 ** 6, 256), (4096, 4, True)), ((1000, 1), (16, 1, False)), ((1025, 1), (16, 2, True))]


@pytest.mark.parametrize("size,want", GATHER_BY_HAND)
def test_gather_add_launch_mirror(size, want):
    E, cus = size
    l = N.gather_add_launch(E, cus)
    assert (N.gather_add_grid(E, 8, cus), l.passes, l.capped) == want


# node_proj: forward / data gradient 128 rows per workgroup, cap 2 x CUs; weight gradient one tile per wave up to 64 tiles, four from there
# on (512 rows per workgroup), cap CUs.  (R, cus) -> grid, passes, capped; wgrad grid, passes, slots, capped
PROJ_BY_HAND = [
    ((1, 256), (1, 1, False, 1, 1, 1, False)),
    ((2048, 256), (16, 1, False, 16, 1, 64, False)),             # 64 tiles: one per wave
    ((2049, 256), (17, 1, False, 5, 4, 20, False)),              # 65 tiles: up to four per wave, 5 workgroups of 20 waves
    ((65536, 256), (512, 1, False, 128, 4, 512, False)),         # forward / dgrad exactly at the cap
    ((65537, 256), (512, 2, True, 129, 4, 516, False)),
    ((131072, 256), (512, 2, True, 256, 4, 1024, False)),        # wgrad exactly at its cap
    ((131073, 256), (512, 3, True, 256, 5, 1024, True)),
    ((13122, 256), (103, 1, False, 26, 4, 104, False)),          # the benchmark's mesh, B = 2
]


@pytest.mark.parametrize("size,want", PROJ_BY_HAND)
def test_node_proj_launch_mirror(size, want):
    R, cus = size
    f, d, w = N.proj_launches(R, cus)
    assert f[1:] == d[1:] and (f.kernel, d.kernel, w.kernel) == ("node_proj_fwd", "node_proj_dgrad", "node_proj_wgrad")
    assert (N.proj_grid(R, N.PROJ_PER_CU, cus), f.passes, f.capped, N.wgrad_grid(R, cus), w.passes, w.slots, w.capped) == want
    assert w.slots == N.wgrad_slots(R, cus)


def test_issue_thresholds_at_256_cus():
    """where each kernel starts to loop at 256 CUs, bf16, 64 features: the table the suite was written from"""
    cus = 256
    first = lambda capped: next(r for r in range(1, 1 << 20) if capped(r))  # noqa: E731
    assert not N.mlp_launch(32768, 1, cus, bwd=True).capped and N.mlp_launch(32769, 1, cus, bwd=True).capped
    assert not N.mlp_launch(131072, 4, cus).capped and N.mlp_launch(131073, 4, cus).capped
    assert not N.gather_add_launch(262144, cus).capped and N.gather_add_launch(262145, cus).capped
    assert not N.segment_sum_launch(131072, 131072, cus).capped and N.segment_sum_launch(131073, 131073, cus).capped
    assert not N.segment_sum_launch(16384, 16384 * 40, cus).capped and N.segment_sum_launch(16385, 16385 * 40, cus).capped
    assert not N.proj_launches(131072, cus)[2].capped and N.proj_launches(131073, cus)[2].capped
    assert first(lambda r: N.proj_launches(r, cus)[0].capped) == 65537


@pytest.mark.parametrize("model", ["graphlam", "hilam"])
def test_caps_grid_at_256_cus(model):
    cus, B = 256, 2
    (h, w), bench = N.smallest_grid_past_caps_of(model, B, 512, 512, cus, processor_layers=1)
    print(f"\n{model}: caps grid {h} x {w}, sizes {vars(N.graph_sizes(h, w))}")
    assert h * w < 512 * 512 and h % 2 and w % 2
    assert N.mesh_levels(h, w) == N.mesh_levels(512, 512) == [6561, 729, 81, 9] == N.graph_sizes(h, w).levels
    table = N.launch_table(model, B, h, w, cus, processor_layers=1)
    assert table.keys() == bench.keys() and N.loop_signature(table) == N.loop_signature(bench)
    s = N.graph_sizes(h, w)
    for count in (B * h * w, B * s.g2m, B * s.m2g, B * s.n_mesh):        # (the mesh's own edge count is the hierarchy's: 2 x 57 616 =
        assert count % 32, count                                         #  32 x 3 601 at every grid; the direct cases have odd tails)
    # the benchmark runs inside the loops, and so does the caps grid; the toy grid runs inside none
    looping = {(n, l.kernel) for n, ls in table.items() for l in ls if l.capped}
    assert {k for _, k in looping} >= {"row_mlp_fwd", "row_mlp_bwd", "edge_gather_add_fwd", "segment_sum", "node_proj_fwd", "node_proj_dgrad",
                                       "node_proj_wgrad"}, looping
    assert looping == {(n, l.kernel) for n, ls in bench.items() for l in ls if l.capped}
    toy = N.launch_table(model, B, 36, 45, cus, processor_layers=1)
    assert not any(l.capped for ls in toy.values() for l in ls)
    shared = set(toy) & set(table)
    assert shared and N.loop_signature({k: toy[k] for k in shared}) != N.loop_signature({k: table[k] for k in shared})
    # 2 x 243 x 288 (the even grid the hierarchy first appears near) has the property too: the search lands at or below its area
    assert N.loop_signature(N.launch_table(model, B, 243, 288, cus, processor_layers=1)) == N.loop_signature(bench)
    assert h * w <= 243 * 288
