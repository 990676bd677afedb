"""
Node-level oracle of the native mesh GNNs (py4cast_amd/graphlam.py, hilam.py, hilamparallel.py): float64 references of the networks' nodes,
a Python mirror of the launch shapes of their kernels (csrc/mlp.hip, nodeproj.hip, graph.hip), and a recorder of the node calls of a
forward / backward -- the helpers of tests/test_gnn_nodes_gpu.py (the device) and tests/test_gnn_nodes_cpu.py (the references and the mirror
themselves, against oracle/graphlam.py, oracle/hilam.py and the launch code written out by hand).

References: float64 functions on rows (R, C) that run on CPU or GPU tensors alike and differentiate through torch autograd; `node()` turns
one into (outputs, gradients) for recorded incoming gradients.  Activations are taken as given (the recorded bf16 tensors, promoted).  A
weight is rounded to bf16 exactly where the kernel reads a bf16 image of it -- the GEMM weights of the bf16 flavour (`gemm_w`); biases and
LayerNorm parameters stay the fp32 values they are.  The fused row MLP feeds its hidden activation SiLU(W1 x + ...) to the second MFMA as
bf16: `row_mlp(..., round_hidden=True)` rounds it there (straight-through in the backward).  With rounding off everything is plain float64.
The batch is folded into the rows as the models fold it (edge lists replicated with node offsets: `fold`).

Launch mirror: `mlp_grid`, `mlp_bwd_slots`, `segment_sum_shape`, `gather_add_grid`, `proj_grid`, `wgrad_grid`, `wgrad_slots` restate the
functions of the same names of the launch code from sizes and the CU count alone; `launch_table` lists, for every leaf node of a model at a
grid, the kernels it launches with (passes per wave, split_log2, partial slots, capped), and `smallest_grid_past_caps_of` searches the
smallest grid with the benchmark's mesh hierarchy whose table loops where the benchmark's loops.
"""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

C = 64      # hidden width of every GNN MLP (config/CLI/model/graphlam.yaml: hidden_dims 64)

# ------------------------------------------------------------------------------------------------ float64 node references


def gemm_w(w, on=True):
    """the weight as a bf16 MFMA reads it (on), as float64"""
    w = w.detach()
    return (w.to(torch.bfloat16) if on else w).double()


def round_bf16(t):
    """t rounded to bf16, straight-through for the gradient"""
    return t + (t.detach().to(torch.bfloat16).double() - t.detach())


def rows_of(t, index):
    """t[index]: the gather of node rows onto edges (its adjoint is segment_sum)"""
    return t.index_select(0, index.long())


def segment_sum(msg, dst, n):
    """out[r] = sum of msg[e] over the edges e with dst[e] == r; receivers without edges get zero"""
    return torch.zeros(n, msg.shape[1], dtype=msg.dtype, device=msg.device).index_add_(0, dst.long(), msg)


def in_degree(dst, n):
    return torch.bincount(dst.long(), minlength=n)


def mean_of_sum(agg, dst, n):
    """mesh_aggr mean: a receiver's sum over its number of incoming edges (1 for a receiver without edges: its sum is zero)"""
    return agg / in_degree(dst, n).clamp_min(1).to(agg.dtype).unsqueeze(1)


def act(v, name):
    if name in (None, "none"):
        return v
    return F.relu(v) if name == "relu" else F.silu(v)


def edge_gather_add(base, a, ia, b, ib, name=None):
    """act(base[e] + a[ia[e]] + b[ib[e]]); each of base, a, b optional"""
    terms = [t for t in (base, None if a is None else rows_of(a, ia), None if b is None else rows_of(b, ib)) if t is not None]
    return act(sum(terms[1:], terms[0]), name)


def linear(x, w, b=None):
    y = x @ w.t()
    return y if b is None else y + b


def ln_res(x, g, b, eps=1e-5, res=None):
    """row LayerNorm over the features, plus a residual"""
    y = F.layer_norm(x, (x.shape[-1],), g, b, eps)
    return y if res is None else y + res


def row_mlp(x, w1, b1, w2, b2, gamma=None, beta=None, eps=1e-5, ga=None, ia=None, gb=None, ib=None, res=None, round_hidden=False):
    """(y, y + res) with y = LN(W2 SiLU(W1 x + b1 [+ ga[ia]] [+ gb[ib]]) + b2).  x may be wider than w1 (zero-padded to the kernel's
    multiple of 16: the first w1.shape[1] features count); w2 may have fewer than 64 rows (the output map, no LayerNorm); ia / ib None:
    row-aligned addends; round_hidden: the hidden activation rounded to bf16, as the second MFMA reads it"""
    pre = linear(x[:, :w1.shape[1]], w1, b1)
    if ga is not None:
        pre = pre + (ga if ia is None else rows_of(ga, ia))
    if gb is not None:
        pre = pre + (gb if ib is None else rows_of(gb, ib))
    h = F.silu(pre)
    if round_hidden:
        h = round_bf16(h)
    y = linear(h, w2, b2)
    if gamma is not None:
        y = F.layer_norm(y, (y.shape[-1],), gamma, beta, eps)
    return y, (None if res is None else y + res)


def node_proj(x, weights, passthrough=False):
    """(x W_1^T, ..., x W_n^T [, x]): n projections of one node tensor; the gradient of the returned x is summed into dx"""
    return tuple(x @ w.t() for w in weights) + ((x,) if passthrough else ())


def mlp_rows(x, P, pre, layer_norm=True, res=None, round_hidden=False):
    """make_mlp's Linear - SiLU - Linear [- LayerNorm] under the parameter names `pre`0.*, `pre`2.*, `pre`3.* [+ res]"""
    y, yr = row_mlp(x, P[pre + "0.weight"], P[pre + "0.bias"], P[pre + "2.weight"], P[pre + "2.bias"],
                    P[pre + "3.weight"] if layer_norm else None, P[pre + "3.bias"] if layer_norm else None, res=res, round_hidden=round_hidden)
    return y if res is None else yr


def interaction_net(send, rec, edge, src, dst, P, pre, update_edges=True, aggr="sum", round_hidden=False):
    """neural-lam's InteractionNet in the concat formulation: the edge MLP on cat[e, x_s[src], x_r[dst]], the aggregation by index_add_,
    the node update on cat[x_r, agg] with residual"""
    msg = mlp_rows(torch.cat([edge, rows_of(send, src), rows_of(rec, dst)], dim=-1), P, pre + "edge_mlp.", round_hidden=round_hidden)
    agg = segment_sum(msg, dst, rec.shape[0])
    if aggr == "mean":
        agg = mean_of_sum(agg, dst, rec.shape[0])
    new = rec + mlp_rows(torch.cat([rec, agg], dim=-1), P, pre + "aggr_mlp.", round_hidden=round_hidden)
    return (new, edge + msg) if update_edges else new


def interaction_net_distributed(send, rec, edge, src, dst, P, pre, update_edges=True, aggr="sum"):
    """the same InteractionNet as the native models run it: the first Linear of the edge MLP distributed over the concat (node projections
    once per node, gathered addends), the receiver half of the node update a row-aligned addend"""
    w0, a0 = P[pre + "edge_mlp.0.weight"], P[pre + "aggr_mlp.0.weight"]
    a, = node_proj(send, [w0[:, C:2 * C]])
    b, part, rec_res = node_proj(rec, [w0[:, 2 * C:], a0[:, :C]], passthrough=True)
    msg, new_edge = row_mlp(edge, w0[:, :C], P[pre + "edge_mlp.0.bias"], P[pre + "edge_mlp.2.weight"], P[pre + "edge_mlp.2.bias"],
                            P[pre + "edge_mlp.3.weight"], P[pre + "edge_mlp.3.bias"], ga=a, ia=src, gb=b, ib=dst, res=edge)
    agg = segment_sum(msg, dst, rec.shape[0])
    if aggr == "mean":
        agg = mean_of_sum(agg, dst, rec.shape[0])
    _, new = row_mlp(agg, a0[:, C:], P[pre + "aggr_mlp.0.bias"], P[pre + "aggr_mlp.2.weight"], P[pre + "aggr_mlp.2.bias"],
                     P[pre + "aggr_mlp.3.weight"], P[pre + "aggr_mlp.3.bias"], ga=part, res=rec_res)
    return (new, new_edge) if update_edges else new


def fold(index, B, ns, nr):
    """an edge list (2, E) replicated over the batch with node offsets, as the models' _edges"""
    return (torch.cat([index[0] + b * ns for b in range(B)]), torch.cat([index[1] + b * nr for b in range(B)]))


def _rep(t, B):
    return t.unsqueeze(0).expand(B, *t.shape).reshape(B * t.shape[0], t.shape[1])


def graphlam_network(x, P, g, aggr="sum", inet=interaction_net):
    """GraphLamMI355X.forward composed of the node references, on a dict P of float64 parameters under the model's names and the graph g
    (oracle/graphlam.py's dict); x (B, n_grid, C_in)"""
    B, N, _ = x.shape
    M = g["mesh_pos"].shape[0]
    f = lambda t: t.to(x.dtype)  # noqa: E731
    es = {k: fold(g[k], B, ns, nr) for k, (ns, nr) in (("g2m", (N, M)), ("m2m", (M, M)), ("m2g", (M, N)))}
    grid = mlp_rows(x.reshape(B * N, -1), P, "grid_embedder.")
    g2m_e, m2g_e, m2m_e = (_rep(mlp_rows(f(g[k + "_feat"]), P, k + "_embedder."), B) for k in ("g2m", "m2g", "m2m"))
    mesh = _rep(mlp_rows(f(g["mesh_pos"]), P, "mesh_embedder."), B)
    mesh = inet(grid, mesh, g2m_e, *es["g2m"], P, "g2m_gnn.", False)
    grid = mlp_rows(grid, P, "encoding_grid_mlp.", res=grid)
    i = 0
    while f"processor.{i}.edge_mlp.0.weight" in P:
        mesh, m2m_e = inet(mesh, mesh, m2m_e, *es["m2m"], P, f"processor.{i}.", True, aggr)
        i += 1
    grid = inet(mesh, grid, m2g_e, *es["m2g"], P, "m2g_gnn.", False)
    return mlp_rows(grid, P, "output_map.", layer_norm=False).reshape(B, N, -1)


def _hilam_encode(x, P, g, inet):
    B, N, _ = x.shape
    Lv = len(g["mesh_pos"])
    nm = [p.shape[0] for p in g["mesh_pos"]]
    f = lambda t: t.to(x.dtype)  # noqa: E731
    es = {"g2m": fold(g["g2m"], B, N, nm[0]), "m2g": fold(g["m2g"], B, nm[0], N)}
    for l in range(Lv):
        es[f"same{l}"] = fold(g["same"][l], B, nm[l], nm[l])
    for l in range(Lv - 1):
        es[f"up{l}"] = fold(g["up"][l], B, nm[l], nm[l + 1])
        es[f"down{l}"] = fold(g["down"][l], B, nm[l + 1], nm[l])
    grid = mlp_rows(x.reshape(B * N, -1), P, "grid_embedder.")
    g2m_e, m2g_e = (_rep(mlp_rows(f(g[k + "_feat"]), P, k + "_embedder."), B) for k in ("g2m", "m2g"))
    levels = [_rep(mlp_rows(f(g["mesh_pos"][l]), P, f"mesh_embedders.{l}."), B) for l in range(Lv)]
    same_e = [_rep(mlp_rows(f(g["same_feat"][l]), P, f"mesh_same_embedders.{l}."), B) for l in range(Lv)]
    up_e = [_rep(mlp_rows(f(g["up_feat"][l]), P, f"mesh_up_embedders.{l}."), B) for l in range(Lv - 1)]
    down_e = [_rep(mlp_rows(f(g["down_feat"][l]), P, f"mesh_down_embedders.{l}."), B) for l in range(Lv - 1)]
    levels[0] = inet(grid, levels[0], g2m_e, *es["g2m"], P, "g2m_gnn.", False)
    grid = mlp_rows(grid, P, "encoding_grid_mlp.", res=grid)
    for l in range(1, Lv):
        levels[l], up_e[l - 1] = inet(levels[l - 1], levels[l], up_e[l - 1], *es[f"up{l - 1}"], P, f"mesh_init_gnns.{l - 1}.")
    return grid, m2g_e, levels, same_e, up_e, down_e, es


def _hilam_decode(x, grid, m2g_e, levels, down_e, es, P, inet):
    B, N, _ = x.shape
    for l in range(len(levels) - 2, -1, -1):
        levels[l] = inet(levels[l + 1], levels[l], down_e[l], *es[f"down{l}"], P, f"mesh_read_gnns.{l}.", False)
    grid = inet(levels[0], grid, m2g_e, *es["m2g"], P, "m2g_gnn.", False)
    return mlp_rows(grid, P, "output_map.", layer_norm=False).reshape(B, N, -1)


def hilam_network(x, P, g, inet=interaction_net):
    """HiLamMI355X.forward composed of the node references (init, per processor layer a down and an up sweep, read-out)"""
    grid, m2g_e, levels, same_e, up_e, down_e, es = _hilam_encode(x, P, g, inet)
    Lv, i = len(levels), 0
    while f"mesh_down_same_gnns.{i}.0.edge_mlp.0.weight" in P:
        d, ds, u, us = (f"mesh_{k}_gnns.{i}." for k in ("down", "down_same", "up", "up_same"))
        levels[-1], same_e[-1] = inet(levels[-1], levels[-1], same_e[-1], *es[f"same{Lv - 1}"], P, f"{ds}{Lv - 1}.")
        for l in range(Lv - 2, -1, -1):
            new, down_e[l] = inet(levels[l + 1], levels[l], down_e[l], *es[f"down{l}"], P, f"{d}{l}.")
            levels[l], same_e[l] = inet(new, new, same_e[l], *es[f"same{l}"], P, f"{ds}{l}.")
        levels[0], same_e[0] = inet(levels[0], levels[0], same_e[0], *es["same0"], P, f"{us}0.")
        for l in range(1, Lv):
            new, up_e[l - 1] = inet(levels[l - 1], levels[l], up_e[l - 1], *es[f"up{l - 1}"], P, f"{u}{l - 1}.")
            levels[l], same_e[l] = inet(new, new, same_e[l], *es[f"same{l}"], P, f"{us}{l}.")
        i += 1
    return _hilam_decode(x, grid, m2g_e, levels, down_e, es, P, inet)


def hilampar_network(x, P, g, inet=interaction_net):
    """HiLamParallelMI355X.forward: HiLAM's encoder / init / read-out around layers that are ONE InteractionNet over all mesh edges, an
    edge MLP per edge set and a node-update MLP per level -- written per edge set, as the native model runs it"""
    grid, m2g_e, levels, same_e, up_e, down_e, es = _hilam_encode(x, P, g, inet)
    Lv, i = len(levels), 0
    sets = [(f"same{l}", l, l) for l in range(Lv)] + [(f"up{l}", l, l + 1) for l in range(Lv - 1)] + [(f"down{l}", l + 1, l) for l in range(Lv - 1)]
    reps = same_e + up_e + down_e
    while f"processor.{i}.edge_mlps.0.0.weight" in P:
        agg, new = [None] * Lv, []
        for k, (name, ls, lr) in enumerate(sets):
            src, dst = es[name]
            msg = mlp_rows(torch.cat([reps[k], rows_of(levels[ls], src), rows_of(levels[lr], dst)], dim=-1), P, f"processor.{i}.edge_mlps.{k}.")
            new.append(reps[k] + msg)
            part = segment_sum(msg, dst, levels[lr].shape[0])
            agg[lr] = part if agg[lr] is None else agg[lr] + part
        levels = [levels[l] + mlp_rows(torch.cat([levels[l], agg[l]], dim=-1), P, f"processor.{i}.aggr_mlps.{l}.") for l in range(Lv)]
        reps, i = new, i + 1
    return _hilam_decode(x, grid, m2g_e, levels, reps[2 * Lv - 1:], es, P, inet)


def leaf(t):
    return None if t is None else t.detach().double().requires_grad_(True)


def node(fn, inputs, dys):
    """fn(*inputs) on float64 leaves of `inputs` (None entries stay None, non-floating tensors and non-tensors pass through):
    (outputs, [gradients]) for the incoming gradients dys (one per output of fn; an output whose dy is None takes none).  fn returns a
    tensor or a tuple of tensors / None."""
    leaves = [leaf(t) if isinstance(t, torch.Tensor) and t.is_floating_point() else t for t in inputs]
    single = not isinstance(dys, (tuple, list))
    with torch.enable_grad():
        ys = fn(*leaves)
        ys = (ys,) if single else tuple(ys)
        dys = (dys,) if single else tuple(dys)
        live = [t for t in leaves if isinstance(t, torch.Tensor) and t.requires_grad]
        # (an output narrower than the kernel's 64 features -- the output map -- takes the first features of the recorded gradient)
        pairs = [(y, d.double()[..., :y.shape[-1]]) for y, d in zip(ys, dys) if y is not None and d is not None and y.requires_grad]
        got = iter(torch.autograd.grad([y for y, _ in pairs], live, [d for _, d in pairs], allow_unused=True))
    grads = [next(got) if isinstance(t, torch.Tensor) and t.requires_grad else None for t in leaves]
    outs = tuple(None if y is None else y.detach() for y in ys)
    return (outs[0] if single else outs), grads


# ------------------------------------------------------------------------------------------------ the launch mirror
# (kernel, passes: tiles / row batches / segment batches one wave takes, split_log2 of a segment sum, partial slots of a parameter-gradient
#  launch, capped: the grid hit its multiple of the CU count -- from there on a wave LOOPS over several passes)
Launch = namedtuple("Launch", "kernel passes split_log2 slots capped")

PER_WAVE_MAX_G = 16      # csrc/mlp.hip: workgroups up to which every wave of row_mlp_bwd leaves its own partial slot


def _cdiv(a, b):
    return -(-a // b)


def mlp_grid(R, per_cu, cus):
    """csrc/mlp.hip mlp_grid: 32-row tiles, four waves (tiles) per workgroup, at most cus x per_cu workgroups"""
    return max(min(_cdiv(_cdiv(R, 32), 4), cus * per_cu), 1)


def mlp_bwd_slots(R, cus):
    G = mlp_grid(R, 1, cus)
    return G if G > PER_WAVE_MAX_G else min(_cdiv(R, 32), 4 * G)


def mlp_launch(R, per_cu, cus, bwd=False):
    G = mlp_grid(R, per_cu, cus)
    return Launch("row_mlp_bwd" if bwd else "row_mlp_fwd", _cdiv(_cdiv(R, 32), 4 * G), None, mlp_bwd_slots(R, cus) if bwd else None,
                  _cdiv(_cdiv(R, 32), 4) > cus * per_cu)


def _ceil_log2(v):
    return max(int(v) - 1, 0).bit_length()


def segment_sum_shape(N, E, chunks, cus):
    """csrc/graph.hip segment_sum_shape: (blocks, lpr_log2, split_log2); lane groups per segment from the mean list length"""
    lpr_log2 = min(_ceil_log2(chunks), 6)
    mean_len = _cdiv(E, N)
    split_log2 = 0
    while split_log2 < 6 - lpr_log2 and (4 << split_log2) < mean_len:
        split_log2 += 1
    spw = (64 >> lpr_log2) >> split_log2
    return min(_cdiv(_cdiv(N, spw), 4), cus * 16), lpr_log2, split_log2


def segment_sum_launch(N, E, cus, chunks=8):
    blocks, lpr_log2, split_log2 = segment_sum_shape(N, E, chunks, cus)
    waves = _cdiv(N, (64 >> lpr_log2) >> split_log2)
    return Launch("segment_sum", _cdiv(waves, 4 * blocks), split_log2, None, _cdiv(waves, 4) > cus * 16)


def gather_add_grid(E, chunks, cus):
    """csrc/graph.hip launch_gather_add: 2 x (64 >> lpr_log2) rows per wave pass, at most cus x 16 workgroups"""
    rpw = 64 >> min(_ceil_log2(chunks), 6)
    return max(min(_cdiv(_cdiv(E, 2 * rpw), 4), cus * 16), 1)


def gather_add_launch(E, cus, chunks=8, bwd=False):
    waves = _cdiv(E, 2 * (64 >> min(_ceil_log2(chunks), 6)))
    return Launch("edge_gather_add_bwd" if bwd else "edge_gather_add_fwd", _cdiv(waves, 4 * gather_add_grid(E, chunks, cus)), None, None,
                  _cdiv(waves, 4) > cus * 16)


def proj_grid(R, per_cu, cus):
    return max(min(_cdiv(_cdiv(R, 32), 4), cus * per_cu), 1)


def wgrad_grid(R, cus):
    """csrc/nodeproj.hip wgrad_grid: one tile per wave up to 64 tiles, four from there on, at most cus workgroups"""
    tiles = _cdiv(R, 32)
    per_wave = 1 if tiles <= 64 else 4
    return max(min(_cdiv(tiles, 4 * per_wave), cus), 1)


def wgrad_slots(R, cus):
    return min(_cdiv(R, 32), 4 * wgrad_grid(R, cus))


PROJ_PER_CU = 2          # csrc/nodeproj.hip: proj_grid(R, 2) at both call sites (forward and data gradient)


def proj_launches(R, cus):
    tiles = _cdiv(R, 32)
    G = proj_grid(R, PROJ_PER_CU, cus)
    capped = _cdiv(tiles, 4) > cus * PROJ_PER_CU
    Gw = wgrad_grid(R, cus)
    return (Launch("node_proj_fwd", _cdiv(tiles, 4 * G), None, None, capped), Launch("node_proj_dgrad", _cdiv(tiles, 4 * G), None, None, capped),
            Launch("node_proj_wgrad", _cdiv(tiles, 4 * Gw), None, wgrad_slots(R, cus), tiles > 64 and _cdiv(tiles, 16) > cus))


def row_mlp_launches(R, cus, n_src=None, n_dst=None):
    """the fused MLP over R rows: forward, backward, and with gathered addends the two segment sums of its pre-activation gradient
    (one segment_sum_pair launch: each half has the shape of its own launch)"""
    t = (mlp_launch(R, 4, cus), mlp_launch(R, 1, cus, bwd=True))
    if n_src is not None:
        t += (segment_sum_launch(n_src, R, cus), segment_sum_launch(n_dst, R, cus))
    return t


def aggregate_launches(N, E, cus):
    return (segment_sum_launch(N, E, cus), gather_add_launch(E, cus))


def node_launches(n, cus):
    """the launches of a recorded leaf node, from its recorded sizes"""
    s = n.sizes
    if n.kind == "row_mlp":
        return row_mlp_launches(s["R"], cus, s.get("n_src"), s.get("n_dst"))
    if n.kind == "node_proj":
        return proj_launches(s["R"], cus)
    if n.kind == "segment_sum":
        return aggregate_launches(s["N"], s["E"], cus)
    return ()


@functools.lru_cache(maxsize=None)
def graph_sizes(H, W):
    """node and edge counts of the mesh graphs of an (H, W) grid (py4cast_amd.graph_build on a unit meshgrid), per sample"""
    from py4cast_amd.graph_build import build_hierarchical_graph, build_mesh_graph

    ys, xs = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    g, h = build_mesh_graph(torch.stack([xs, ys])), build_hierarchical_graph(torch.stack([xs, ys]))
    deg = lambda e, n: (int(in_degree(e[1], n).min()), int(in_degree(e[1], n).max()))  # noqa: E731
    return SimpleNamespace(n_grid=H * W, n_mesh=g.n_mesh, g2m=g.g2m.shape[1], m2m=g.m2m.shape[1], m2g=g.m2g.shape[1], levels=list(h.n_mesh),
                           same=[e.shape[1] for e in h.same], up=[e.shape[1] for e in h.up], hi_g2m=h.g2m.shape[1], hi_m2g=h.m2g.shape[1],
                           degrees={"g2m": deg(g.g2m, g.n_mesh), "m2g": deg(g.m2g, H * W), "same0": deg(h.same[0], h.n_mesh[0]),
                                    **({"up0": deg(h.up[0], h.n_mesh[1])} if h.up else {})})


def mesh_levels(H, W, refine=3):
    """the hierarchy's level sizes from the grid's extent alone (graph_build.build_hierarchical_graph)"""
    n = refine ** int(math.log(max(H, W)) / math.log(refine)) // refine
    sizes = []
    while n >= 2:
        sizes.append(n * n)
        n //= refine
    return sizes or [4]


def _inet_entries(t, pre, ns, nr, E, same, cus):
    if same:
        t[pre + "edge_mlp.proj1"] = proj_launches(nr, cus)
    else:
        t[pre + "edge_mlp.proj1"] = proj_launches(ns, cus)
        t[pre + "edge_mlp.proj2"] = proj_launches(nr, cus)
    t[pre + "edge_mlp"] = row_mlp_launches(E, cus, ns, nr)
    t[pre + "edge_mlp.aggregate"] = aggregate_launches(nr, E, cus)
    t[pre + "aggr_mlp"] = row_mlp_launches(nr, cus)


def launch_table(model_name, B, H, W, cus, processor_layers=None):
    """{leaf node: its launches} of the bf16 flavour with gradient buffers (the benchmark's route) at a (B, H, W) input, from sizes alone"""
    s = graph_sizes(H, W)
    t = {}
    R = B * s.n_grid
    t["grid_embedder"] = t["encoding_grid_mlp"] = t["output_map"] = row_mlp_launches(R, cus)
    if model_name == "graphlam":
        P = 4 if processor_layers is None else processor_layers
        M = B * s.n_mesh
        for k, rows in (("g2m", s.g2m), ("m2g", s.m2g), ("m2m", s.m2m), ("mesh", s.n_mesh)):        # static features: not batched
            t[f"{k}_embedder"] = row_mlp_launches(rows, cus)
        _inet_entries(t, "g2m_gnn.", R, M, B * s.g2m, False, cus)
        for i in range(P):
            _inet_entries(t, f"processor.{i}.", M, M, B * s.m2m, True, cus)
        _inet_entries(t, "m2g_gnn.", M, R, B * s.m2g, False, cus)
        return t
    P = 4 if processor_layers is None else processor_layers
    nm, Lv = s.levels, len(s.levels)
    t["g2m_embedder"], t["m2g_embedder"] = row_mlp_launches(s.hi_g2m, cus), row_mlp_launches(s.hi_m2g, cus)
    for l in range(Lv):
        t[f"mesh_embedders.{l}"], t[f"mesh_same_embedders.{l}"] = row_mlp_launches(nm[l], cus), row_mlp_launches(s.same[l], cus)
    for l in range(Lv - 1):
        t[f"mesh_up_embedders.{l}"] = t[f"mesh_down_embedders.{l}"] = row_mlp_launches(s.up[l], cus)
    _inet_entries(t, "g2m_gnn.", R, B * nm[0], B * s.hi_g2m, False, cus)
    _inet_entries(t, "m2g_gnn.", B * nm[0], R, B * s.hi_m2g, False, cus)
    for l in range(Lv - 1):
        _inet_entries(t, f"mesh_init_gnns.{l}.", B * nm[l], B * nm[l + 1], B * s.up[l], False, cus)
        _inet_entries(t, f"mesh_read_gnns.{l}.", B * nm[l + 1], B * nm[l], B * s.up[l], False, cus)
    if model_name == "hilam":
        for i in range(P):
            for l in range(Lv):
                for k in ("down_same", "up_same"):
                    _inet_entries(t, f"mesh_{k}_gnns.{i}.{l}.", B * nm[l], B * nm[l], B * s.same[l], True, cus)
            for l in range(Lv - 1):
                _inet_entries(t, f"mesh_down_gnns.{i}.{l}.", B * nm[l + 1], B * nm[l], B * s.up[l], False, cus)
                _inet_entries(t, f"mesh_up_gnns.{i}.{l}.", B * nm[l], B * nm[l + 1], B * s.up[l], False, cus)
        return t
    assert model_name == "hilampar", model_name
    sets = [(l, l, s.same[l]) for l in range(Lv)] + [(l, l + 1, s.up[l]) for l in range(Lv - 1)] + [(l + 1, l, s.up[l]) for l in range(Lv - 1)]
    for i in range(P):
        for k, (ls, lr, E) in enumerate(sets):
            pre = f"processor.{i}.edge_mlps.{k}"
            t[pre + ".proj1"] = proj_launches(B * nm[lr if ls == lr else ls], cus)
            if ls != lr:
                t[pre + ".proj2"] = proj_launches(B * nm[lr], cus)
            t[pre] = row_mlp_launches(B * E, cus, B * nm[ls], B * nm[lr])
            t[pre + ".aggregate"] = aggregate_launches(B * nm[lr], B * E, cus)
        for l in range(Lv):
            t[f"processor.{i}.aggr_mlps.{l}.proj0"] = proj_launches(B * nm[l], cus)
            t[f"processor.{i}.aggr_mlps.{l}"] = row_mlp_launches(B * nm[l], cus)
    return t


def loop_signature(table):
    """what of a launch table decides the code path: per node and launch, the kernel, whether a wave loops past the cap, and the split"""
    return {name: tuple((l.kernel, l.capped, l.split_log2) for l in ls) for name, ls in table.items()}


def smallest_grid_past_caps_of(model_name, B, H, W, cus, processor_layers=None):
    """the smallest (by area, then height) grid with ODD height and width -- so that no row, edge or node count is a multiple of 32 -- whose
    mesh hierarchy is that of (H, W) and whose every launch loops / does not loop and splits as at (B, H, W); and the table of (B, H, W).
    (The hierarchy and the grid-row launches are screened from sizes alone; the graph is built only for the grids that pass.)"""
    want = launch_table(model_name, B, H, W, cus, processor_layers)
    sig, levels = loop_signature(want), mesh_levels(H, W)
    rows_sig = loop_signature({"rows": row_mlp_launches(B * H * W, cus) + proj_launches(B * H * W, cus)})
    lo = 3 ** int(math.log(max(H, W)) / math.log(3))
    grids = sorted(((h, w) for h in range(3, H + 1, 2) for w in range(max(h, lo | 1), W + 1, 2)), key=lambda g: (g[0] * g[1], g[0]))
    for h, w in grids:
        if mesh_levels(h, w) != levels or loop_signature({"rows": row_mlp_launches(B * h * w, cus) + proj_launches(B * h * w, cus)}) != rows_sig:
            continue
        if loop_signature(launch_table(model_name, B, h, w, cus, processor_layers)) == sig:
            return (h, w), want
    return (H, W), want


# ------------------------------------------------------------------------------------------------ the recorder

KINDS = ("row_mlp", "node_proj", "segment_sum", "gather_add", "ln", "linear", "flinear", "mlp", "inet", "edge_messages", "node_update")
LEAF_KINDS = ("row_mlp", "node_proj", "segment_sum", "gather_add", "ln", "linear", "flinear")


class Node:
    """one recorded call: kind, name, module (the live layer of a composed node), args (operand clones; a parameter operand is kept as
    ("param", name, shape, strides, offset into the parameter)), opts, outs (clones of the outputs), dys (the gradient each output
    received), parent (index of the enclosing composed node), src ({operand: (producer node index, output slot)}), sizes, launches"""

    def __init__(self, kind, name, module, args, opts, parent):
        self.kind, self.name, self.module, self.args, self.opts, self.parent = kind, name, module, args, opts, parent
        self.outs, self.dys, self.src, self.src_leaf, self.sizes, self.launches = [], [], {}, {}, {}, ()

    @property
    def out(self):
        return self.outs[0]

    @property
    def dy(self):
        return self.dys[0]


def _c(t):
    return None if t is None else t.detach().clone()


class _FunctionalProxy:
    """torch.nn.functional as a model module sees it, with `linear` recorded (the fp32 flavour's library GEMMs)"""

    def __init__(self, linear):
        self.linear = linear

    def __getattr__(self, name):
        return getattr(F, name)


class Recorder:
    """``with Recorder(model, cus) as rec: model(x).backward(dy)``: rec.nodes in call order.  Wraps the entry points as the models call
    them -- ops_mlp.row_mlp, ops_nodeproj.node_proj, ops_graph.aggregate_sum / edge_gather_add, ops_rows.row_linear / row_layer_norm,
    torch.nn.functional.linear as graphlam / hilamparallel see it -- and the composed calls graphlam._run (the embedders, the output map;
    the static-feature embeddings through cached_static_embeddings), InteractionNet.forward, hilamparallel._edge_messages / _node_update.
    The calls themselves are untouched: same arguments, same kernels."""

    def __init__(self, model, cus):
        self.model, self.cus = model, cus
        self.nodes = []
        self.names = {id(m): n for n, m in model.named_modules()}
        self.pnames = {id(p): n for n, p in model.named_parameters()}
        self._depth = 0
        self._stack = []
        self._made = {}          # id(output tensor) -> (node index, slot): the outermost node that returned it
        self._made_leaf = {}     # ... -> (leaf node index, slot): the leaf call that produced it
        self._count = {}

    def __getitem__(self, name):
        got = [n for n in self.nodes if n.name == name]
        assert len(got) == 1, (name, len(got))
        return got[0]

    def of(self, *kinds):
        return [n for n in self.nodes if n.kind in kinds]

    def leaves(self):
        return self.of(*LEAF_KINDS)

    def inside(self, node):
        return [n for n in self.nodes if n.parent == node.index]

    # -------------------------------------------------------------- bookkeeping
    def param_ref(self, t):
        """("param", name, shape, strides, offset) if t is a parameter of the model or a view of one, else None"""
        if not isinstance(t, torch.Tensor):
            return None
        base = t._base if t._base is not None else t
        name = self.pnames.get(id(base))
        return None if name is None else ("param", name, tuple(t.shape), tuple(t.stride()), t.storage_offset() - base.storage_offset())

    def _arg(self, v):
        if isinstance(v, (list, tuple)):
            return [self._arg(u) for u in v]
        return self.param_ref(v) or (_c(v) if isinstance(v, torch.Tensor) else v)

    def _begin(self, kind, name, module, args, opts):
        if name in self._count:       # (a module applied twice -- no model here does -- would still get distinct names)
            self._count[name] += 1
            name = f"{name}#{self._count[name]}"
        else:
            self._count[name] = 0
        node = Node(kind, name, module, {k: self._arg(v) for k, v in args.items()}, opts, self._stack[-1] if self._stack else None)
        for k, v in args.items():
            for j, u in enumerate(v if isinstance(v, (list, tuple)) else [v]):
                key = k if not isinstance(v, (list, tuple)) else f"{k}{j}"
                if isinstance(u, torch.Tensor) and id(u) in self._made:
                    node.src[key] = self._made[id(u)]
                if isinstance(u, torch.Tensor) and id(u) in self._made_leaf:
                    node.src_leaf[key] = self._made_leaf[id(u)]
        return node

    def _place(self, node):
        node.index = len(self.nodes)
        self.nodes.append(node)

    def _outputs(self, node, outs, skip=()):
        """record the outputs (a tensor, or a tuple with None entries) and hook the gradient each receives; `skip`: tensors that are an
        operand handed back as it is (no output of this node)"""
        outs = outs if isinstance(outs, tuple) else (outs,)
        node.outs = [None if (o is None or any(o is s for s in skip)) else _c(o) for o in outs]
        node.dys = [None] * len(outs)
        for j, o in enumerate(outs):
            if node.outs[j] is None:
                continue
            if o.requires_grad:
                o.register_hook(lambda g, j=j: node.dys.__setitem__(j, None if g is None else g.detach().clone()))
            self._made[id(o)] = (node.index, j)
            if node.kind in LEAF_KINDS:
                self._made_leaf[id(o)] = (node.index, j)
            self._keep.append(o)          # (keeps the object alive: a recycled id must not be taken for this output)

    def _leaf(self, kind, name, args, opts, sizes, orig, *a, skip=(), **kw):
        if self._depth:
            return orig(*a, **kw)
        node = self._begin(kind, name, None, args, opts)
        node.sizes = sizes
        node.launches = node_launches(node, self.cus)
        self._place(node)
        self._depth += 1
        try:
            out = orig(*a, **kw)
        finally:
            self._depth -= 1
        self._outputs(node, out, skip)
        return out

    def _owner(self, w, strip=2):
        """the module path of a parameter operand: 'g2m_gnn.edge_mlp.0.weight' -> 'g2m_gnn.edge_mlp'"""
        ref = self.param_ref(w)
        return None if ref is None else ref[1].rsplit(".", strip)[0]

    def _composite(self, kind, name, module, args, opts, orig, *a, **kw):
        node = self._begin(kind, name, module, args, opts)
        self._place(node)                 # (takes its place in call order before its inner nodes)
        self._stack.append(node.index)
        try:
            y = orig(*a, **kw)
        finally:
            self._stack.pop()
        self._outputs(node, y)            # (a composed node's output is its last inner node's: the composed node wins the edge)
        return y

    # -------------------------------------------------------------- the wrappers
    def __enter__(self):
        from py4cast_amd import graphlam as GL
        from py4cast_amd import hilam as HL
        from py4cast_amd import hilamparallel as HP
        from py4cast_amd import ops_graph as G
        from py4cast_amd import ops_mlp as M
        from py4cast_amd import ops_nodeproj as NP
        from py4cast_amd import ops_rows as R

        rec, self._keep = self, []
        o = SimpleNamespace(row_mlp=M.row_mlp, node_proj=NP.node_proj, aggregate=G.aggregate_sum, gather=G.edge_gather_add, rlin=R.row_linear,
                            rln=R.row_layer_norm, run=GL._run, inet=GL.InteractionNet.forward, em=HP._edge_messages, nu=HP._node_update)
        self.orig = o

        def producer_name(t, fallback):
            got = rec._made_leaf.get(id(t)) or rec._made.get(id(t))
            return fallback if got is None else rec.nodes[got[0]].name

        def row_mlp(x, w1, b1, w2, b2, gamma=None, beta=None, eps=1e-5, ga=None, gb=None, edges=None, res=None, want_out=True,
                    grads_in_place=False):
            args = dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, gamma=gamma, beta=beta, ga=ga, gb=gb, res=res)
            opts = dict(eps=eps, edges=edges, want_out=want_out, res_is_x=res is x, grads_in_place=grads_in_place)
            sizes = {"R": x.shape[0], "K": x.shape[1], "O": w2.shape[0]}
            if edges is not None and (ga is not None or gb is not None):
                sizes.update(n_src=edges.n_src, n_dst=edges.n_dst)
            return rec._leaf("row_mlp", rec._owner(w1), args, opts, sizes, o.row_mlp, x, w1, b1, w2, b2, gamma, beta, eps, ga, gb, edges, res,
                             want_out, grads_in_place)

        def node_proj(x, weights, grads_in_place=True, passthrough=False):
            weights = list(weights)
            ref = rec.param_ref(weights[0])
            name = f"{ref[1].rsplit('.', 2)[0]}.proj{ref[4] // C}"
            native = bool(grads_in_place and NP.node_proj_ok(x, weights) and torch.is_grad_enabled() and all(w.requires_grad for w in weights)
                          and all(g is not None and g is not False and g.stride(1) == 1 for g in (R.grad_view(w) for w in weights)))
            opts = dict(grads_in_place=grads_in_place, passthrough=passthrough, native=native, n=len(weights))
            return rec._leaf("node_proj", name, dict(x=x, weights=weights), opts, {"R": x.shape[0], "n": len(weights)}, o.node_proj, x, weights,
                             grads_in_place, passthrough, skip=(x,))

        def aggregate_sum(msg, edges):
            name = producer_name(msg, "aggregate") + ".aggregate"
            return rec._leaf("segment_sum", name, dict(msg=msg), dict(edges=edges), {"N": edges.n_dst, "E": edges.E}, o.aggregate, msg, edges)

        def edge_gather_add(base, a, b, edges, act=None):
            name = producer_name(base, "gather") + ".gather_add"
            return rec._leaf("gather_add", name, dict(base=base, a=a, b=b), dict(edges=edges, act=act), {"E": edges.E}, o.gather, base, a, b, edges, act)

        def row_linear(x, w, b=None, grads_in_place=False):
            ref = rec.param_ref(w)
            name = f"{ref[1].rsplit('.', 1)[0]}.linear{ref[4] // C if ref[4] else ''}" if ref else "linear"
            return rec._leaf("linear", name, dict(x=x, w=w, b=b), dict(grads_in_place=grads_in_place), {"R": x.shape[0]}, o.rlin, x, w, b, grads_in_place)

        def row_layer_norm(x, gamma, beta, eps=1e-5, res=None, mask=None):
            name = rec._owner(gamma, 1) or "ln"
            return rec._leaf("ln", name, dict(x=x, g=gamma, b=beta, res=res), dict(eps=eps), {"R": x.shape[0]}, o.rln, x, gamma, beta, eps, res, mask)

        def f_linear(x, w, b=None):
            ref = rec.param_ref(w)
            name = f"{ref[1].rsplit('.', 1)[0]}.flinear{ref[4] // C if ref[4] else ''}" if ref else "flinear"
            return rec._leaf("flinear", name, dict(x=x, w=w, b=b), {}, {"R": x.shape[0]}, F.linear, x, w, b)

        def _run(mlp, x, res=None, keep_pad=False):
            if rec._depth:
                return o.run(mlp, x, res, keep_pad)
            first = mlp[0] if not isinstance(mlp[0], torch.nn.SiLU) else mlp[1]
            name = rec.names.get(id(mlp)) or (rec.names[id(first)].rsplit(".", 1)[0] + ".tail")     # (edge_mlp[2:]: a slice of a Sequential)
            return rec._composite("mlp", name + ".mlp", mlp, dict(x=x, res=res), dict(keep_pad=keep_pad, res_is_x=res is x), o.run, mlp, x, res, keep_pad)

        def inet_forward(mod, send_rep, rec_rep, edge_rep, edges):
            return rec._composite("inet", rec.names[id(mod)], mod, dict(send=send_rep, rec=rec_rep, edge=edge_rep),
                                  dict(edges=edges, same=send_rep is rec_rep), o.inet, mod, send_rep, rec_rep, edge_rep, edges)

        def _edge_messages(mlp, send, rec_, edge_rep, edges):
            return rec._composite("edge_messages", rec.names[id(mlp)] + ".messages", mlp, dict(send=send, rec=rec_, edge=edge_rep),
                                  dict(edges=edges, same=send is rec_), o.em, mlp, send, rec_, edge_rep, edges)

        def _node_update(mlp, rec_, agg):
            return rec._composite("node_update", rec.names[id(mlp)] + ".update", mlp, dict(rec=rec_, agg=agg), {}, o.nu, mlp, rec_, agg)

        self._mp = mp = pytest.MonkeyPatch()
        mp.setattr(M, "row_mlp", row_mlp)
        mp.setattr(NP, "node_proj", node_proj)
        mp.setattr(G, "aggregate_sum", aggregate_sum)
        mp.setattr(G, "edge_gather_add", edge_gather_add)
        mp.setattr(R, "row_linear", row_linear)
        mp.setattr(R, "row_layer_norm", row_layer_norm)
        proxy = _FunctionalProxy(f_linear)
        mp.setattr(GL, "F", proxy)
        mp.setattr(HP, "F", proxy)
        for mod in (GL, HL, HP):
            mp.setattr(mod, "_run", _run)
        mp.setattr(GL.InteractionNet, "forward", inet_forward)
        mp.setattr(HP, "_edge_messages", _edge_messages)
        mp.setattr(HP, "_node_update", _node_update)
        return self

    def undo(self):
        self._mp.undo()
        self._keep = []
        self._made, self._made_leaf = {}, {}

    def __exit__(self, exc_type, exc, tb):
        self.undo()
        return False
