"""
The mesh GNNs (py4cast_amd/graphlam.py, hilam.py, hilamparallel.py) node by node, past the launch caps of their kernels: one forward /
backward of GraphLamMI355X / HiLamMI355X / HiLamParallelMI355X under tests/gnn_nodes.py's recorder, then for every recorded node -- the fused
row MLPs (csrc/mlp.hip), the node projections (csrc/nodeproj.hip), the segment sums and gathers (csrc/graph.hip), in the fp32 flavour the row
LayerNorms, row Linears and library Linears, and the composed calls (embedder / output MLPs, InteractionNets, HiLAMParallel's edge messages
and node updates) -- the checks below.  MEASURED VALUES: see the end of this docstring.

Cases (B = 2; LayerNorm gammas / betas moved off 1 / 0 by +-(0.1 ... 0.3)): graphlam-toy-bf16 / -f32 (36 x 45, mesh_aggr sum),
graphlam-toy-mean-bf16, hilam-3lev-bf16 / -f32 (81 x 96: levels [729, 81, 9], processor_layers 2), hilampar-3lev-bf16, and graphlam-caps-bf16 /
hilam-caps-bf16: yaml widths, 69 -> 60 channels, processor_layers 1 (the loops are per kernel, not per layer), on the grid of
gnn_nodes.smallest_grid_past_caps_of: the smallest grid of odd height and width (no row, edge or node count a multiple of 32, the mesh's own
2 x 57 616 edges apart) with the benchmark's mesh hierarchy [6561, 729, 81, 9] on which every launch loops past its cap / does not, and
splits its segments, exactly as at the benchmark's 2 x 512 x 512 -- with the CU count read from the device.

The bf16 cases run WITH gradient buffers (every .grad zero-filled before the step), the benchmark's route: only then do node_proj's own
kernels, p4c_row_mlp_bwd_accumulate and the deferred reduction queue run; without buffers node_proj falls back to one ops_rows.row_linear per
block.  The fp32 cases run with .grad None (nothing there adds in place).

* replay: each node alone, on its recorded operands and incoming gradients with fresh parameter leaves (zero-filled buffers where the case
  has them), gives the in-network outputs BIT FOR BIT, and replayed twice the same gradients bit for bit -- the partial-slot reductions past
  the cap and the deferred queue included.  bf16: NO node is exempt.  fp32: only nodes that run a library GEMM (kind `flinear`, and the
  composed nodes around one) are exempt and held to 1e-5 / 1e-4 instead; the list is printed;
* float64, single-kernel nodes (segment_sum and its adjoint gather, gather_add, row LayerNorm, row Linear, node_proj) at the project's bars:
  bf16 maps <= 6e-3 of the largest magnitude per element and <= 3e-3 in the 2-norm, GEMM weight gradients <= 5e-4, LayerNorm dgamma / dbeta
  <= 2e-3; fp32 flavour outputs <= 1e-5, gradients <= 1e-4.  The adjoint of segment_sum is a pure gather: exact;
* float64, composed nodes (the fused row MLP against gnn_nodes.row_mlp with round_hidden, the embedder MLPs, InteractionNets, edge messages,
  node updates against the concat formulation): COMPOSED_BARS, each at most twice the worst measured value and never above the unit tests'
  1.5e-2 (outputs) / 3e-2 (gradients);
* row-wise: for every node with row outputs, every single row's error relative to that row's reference norm stays within ROW_BARS (at most
  twice the worst measured row); rows whose reference norm is below 1e-3 of the mean are skipped and must be <= 1 % of the rows.  This is
  the check a wrong row at a tile tail, or at the seam between a wave's tiles, cannot pass;
* launch table: every node's recorded sizes give gnn_nodes.launch_table's entry (from the grid alone); the caps cases have the loop
  signature of 2 x 512 x 512, computed without building that model; the toy table differs from it;
* wiring, bit for bit: the gradient every leaf's output received is what the replays of its consumers produced (their sum; with more than
  two terms in one of the orders autograd may have taken): edge MLP dpre -> segment_sum_pair -> the node projections' outputs, node_proj dx
  with the passthrough residual summed inside the launch, `res is x` folding dx + dy_res, aggregate_sum's adjoint gather, level to level
  through HiLAM's init / down / up / read-out sweeps; static embeddings: the sum over the batch of their consumer's gradient; the output
  map's dy is the network's, zero in the padding features; the network's dx is the grid embedder's.  Every p.grad equals the leaf replays',
  every parameter -- or column block: edge_mlp.0.weight [:, :C], [:, C:2C], [:, 2C:], aggr_mlp.0.weight [:, :C], [:, C:] -- belongs to
  exactly one leaf; node and parameter counts asserted (COUNTS);
* sink route (the four toy bf16 cases): every .grad pre-filled, then the step with GRADS_IN_PLACE, and again under FlatDDP with a non-zero
  flat buffer: p.grad = prefill + gradient BIT FOR BIT -- csrc/nodeproj.hip's grad_reduce_batch_kernel forms the whole sum of a job's
  partial slots in registers (the order of mlp.hip's own reduction) and adds it to the buffer once, so the queue forms the sum before
  adding -- and p4c_grad_reduce_pending() is 0 afterwards.  The gradient it is held against bit for bit is the zero-filled-buffer run's
  (the same kernels).  The `.grad is None` run is NO bit-for-bit reference here, nor one to 2e-6: without buffers ops_nodeproj.node_proj
  falls back to one ops_rows.row_linear per block (below 4096 rows the library's bf16 GEMM), the projections already differ by a bf16
  rounding in the forward, and so does everything after them; that run is made, its worst parameter gradient against the buffer run is
  printed (measured 1.9e-2, hilam-3lev-bf16) and held to the unit tests' 3e-2.

Direct kernel cases past each cap (sizes from the CU count, odd tails), against float64 with the row-wise check: row_mlp at
R = 128 x CUs x 2 + 17 and 512 x CUs + 33 (K 16 / 64 / 80, outputs 64 / 60, gathered and row-aligned addends, res / res is x, both reduction
routes); segment_sum bf16 and fp32 at N past the cap for split 0 (mean list <= 4) and the largest split (mean > 32), with empty receivers
and one receiver holding 5 % of the edges; segment_sum_pair bit for bit against its two launches; edge_gather_add forward and backward past
its cap with each activation; node_proj n = 1, 2, 3 past proj_grid's and wgrad_grid's caps.

Measured on one MI355X (256 CUs).  The caps grid found: 2 x 141 x 465 for both models (131 130 grid rows -- the fused MLP's forward cap is
131 072 --, levels [6561, 729, 81, 9], per sample 182 627 g2m, 57 616 m2m and 262 260 m2g edges, in-degrees g2m 23-32, same 3-8, up 9, m2g 4);
2 x 243 x 288 has the benchmark's loop signature too.  The benchmark's launch table (2 x 512 x 512, GraphLam; passes per wave, * = loops past
the cap, sN = split_log2, [partial slots]): grid_embedder / encoding_grid_mlp / output_map / m2g_gnn.aggr_mlp row_mlp_fwd 4* row_mlp_bwd 16*
[256]; g2m_embedder 6* / 23*; m2g_embedder 8* / 32*; m2m_embedder 1 / 2*; mesh_embedder 1 / 1 [52]; g2m_gnn.edge_mlp 12* / 45* + segment sums
4* s0 (senders), 1 s3 (receivers); m2g_gnn.edge_mlp 16* / 64* + 1 s3, 4* s0; processor.i.edge_mlp 1 / 4* + 1 s2, 1 s2; the mesh's aggr_mlp 1 / 1
[103]; aggregates g2m 1 s3 + gather 6*, m2g 4* s0 + gather 8*, m2m 1 s2 + gather 1; node_proj on the grid fwd / dgrad 8* wgrad 16* [1024], on the
mesh 1 / 1 / 4 [104].  HiLAM adds the levels' own small launches (1 pass, per-wave slots on the upper levels).
Nodes / leaves / parameters: graphlam-toy-bf16 46 / 33 / 112 (19 row_mlp, 8 node_proj, 6 segment_sum; 7 mlp, 6 inet), -f32 105 / 80 / 112
(6 segment_sum, 6 gather_add, 18 ln, 50 flinear; 19 mlp, 6 inet), -mean-bf16 36 / 25 / 88, hilam-3lev-bf16 174 / 133 / 400, -f32 397 / 304 /
400, hilampar-3lev-bf16 148 / 107 / 280, graphlam-caps-bf16 31 / 21 / 76, hilam-caps-bf16 162 / 121 / 376.  Exempt from bit-identity: bf16
none; fp32 every `flinear` (library GEMM) and the mlp / inet nodes around one, nothing else (segment_sum, gather_add and ln are held).
Worst node over the six bf16 cases and the direct cases / bar: bf16 maps 3.8e-3 / 6e-3 per element, 2.4e-3 / 3e-3 in the 2-norm; GEMM dW
1.7e-7 / 5e-4.  Composed (bar <= 2 x worst, <= 1.5e-2 / 3e-2): row_mlp y 6.4e-3 / 1.2e-2, dx 5.0e-3 / 9.9e-3, dW 4.9e-3 / 9.8e-3, db 4.5e-3 /
9.0e-3, daddend 3.2e-3 / 6.3e-3; mlp y 1.8e-3 / 3.6e-3, dx 4.4e-3 / 8.7e-3, dparam 4.4e-3 / 8.7e-3; inet (and edge messages, node updates)
y 3.4e-3 / 6.8e-3, dx 6.5e-3 / 1.29e-2, dparam 9.8e-3 / 1.95e-2.  Worst single row / bar: single-kernel rows 5.7e-3 / 1.1e-2, node_proj
rows 2.6e-3 / 5.2e-3, row_mlp rows 8.4e-3 / 1.6e-2, composed rows 5.8e-3 / 1.15e-2; gradient rows against the mean row norm: row_mlp 2.7e-2 /
5.3e-2, node_proj 1.2e-2 / 2.3e-2.  fp32 flavour: outputs 4.5e-7 / 1e-5, gradients 2.6e-6 / 1e-4, rows 1.7e-6 / 3.4e-6.
The whole file (68 tests) takes 19 s on one MI355X.

What the suite found: no defect in a kernel or wrapper.  (In the tests' own code: autograd may hand a parameter a VIEW of a larger buffer as
its .grad -- ops_rows' dgamma / dbeta pair -- so a region of a .grad is addressed from the gradient's own storage offset: Leaves.grad.)
"""
import itertools
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gnn_nodes as N  # noqa: E402

pytestmark = pytest.mark.gpu

BENCH = (2, 512, 512)
# name -> model, (H, W) or None (the caps grid, searched), flavour, mesh_aggr, processor_layers, (cin, cout)
CASES = {
    "graphlam-toy-bf16": ("graphlam", (36, 45), "bf16", "sum", 4, (13, 5)),
    "graphlam-toy-f32": ("graphlam", (36, 45), "f32", "sum", 4, (13, 5)),
    "graphlam-toy-mean-bf16": ("graphlam", (36, 45), "bf16", "mean", 2, (13, 5)),
    "hilam-3lev-bf16": ("hilam", (81, 96), "bf16", "sum", 2, (11, 4)),
    "hilam-3lev-f32": ("hilam", (81, 96), "f32", "sum", 2, (11, 4)),
    "hilampar-3lev-bf16": ("hilampar", (81, 96), "bf16", "sum", 2, (11, 4)),
    "graphlam-caps-bf16": ("graphlam", None, "bf16", "sum", 1, (69, 60)),
    "hilam-caps-bf16": ("hilam", None, "bf16", "sum", 1, (69, 60)),
}

# composed nodes: quantity -> bar (2-norm, relative); at most twice the worst measured value, never above 1.5e-2 (outputs) / 3e-2 (gradients)
COMPOSED_BARS = {
    "row_mlp y": 1.2e-2, "row_mlp dx": 9.9e-3, "row_mlp dW": 9.8e-3, "row_mlp db": 9.0e-3, "row_mlp daddend": 6.3e-3,
    "mlp y": 3.6e-3, "mlp dx": 8.7e-3, "mlp dparam": 8.7e-3,
    "inet y": 6.8e-3, "inet dx": 1.29e-2, "inet dparam": 1.95e-2,
}
# worst single row: outputs relative to that row's reference norm, gradient rows relative to the mean row norm (Tally.rows); at most twice
# the worst measured row -- a maximum over up to 10^6 rows, where a garbled row is off by about 1
ROW_BARS = {"single-kernel rows": 1.1e-2, "node_proj rows": 5.2e-3, "row_mlp rows": 1.6e-2, "row_mlp grad rows": 5.3e-2, "node_proj grad rows": 2.3e-2,
            "composed rows": 1.15e-2, "fp32 rows": 3.4e-6}
# case -> (nodes, leaves, parameters)
COUNTS = {"graphlam-toy-bf16": (46, 33, 112), "graphlam-toy-f32": (105, 80, 112), "graphlam-toy-mean-bf16": (36, 25, 88),
          "hilam-3lev-bf16": (174, 133, 400), "hilam-3lev-f32": (397, 304, 400), "hilampar-3lev-bf16": (148, 107, 280),
          "graphlam-caps-bf16": (31, 21, 76), "hilam-caps-bf16": (162, 121, 376)}

UNIT_OUT, UNIT_GRAD = 1.5e-2, 3e-2      # the kernel unit tests' bars (tests/test_widen_gpu.py): no bar here may be wider


def cus_of(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def same(got, want, what):
    assert got is not None and want is not None, f"{what}: missing ({got is None}, {want is None})"
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError(f"{what}: not bit-identical ({int((d > 0).sum())} elements differ, max {float(d.max()):.3e})")


class Tally:
    """collects every bar's worst value and every miss, so that one run reports them all"""

    def __init__(self, case):
        self.case, self.worst, self.missed = case, {}, []

    def bar(self, v, limit, what, key, cap=None):
        w = self.worst.get(key)
        if w is None or v > w[0]:
            self.worst[key] = (v, limit, what)
        if limit is None and cap is not None:
            limit = cap               # a bar not yet set from a measurement: the unit tests' bar holds meanwhile
        if limit is not None and not v <= limit:
            self.missed.append(f"{what}: {v:.3e} > {limit:.1e} [{key}]")

    def rows(self, got, ref, what, key, limit, own=True):
        """every single row's error.  own: relative to that row's reference norm (outputs: rows after a LayerNorm have norm about 8);
        rows of (almost) no reference norm -- below 1e-3 of the mean -- are skipped, must be <= 1 % of the rows, and are held against the mean
        norm instead.  not own (gradient rows: a row of dx = W^T dpre is a sum that may cancel to nothing, a sender may have no edge):
        every row's error relative to the MEAN row norm -- a garbled row is off by about one mean norm either way."""
        got, ref = got.detach().double(), ref.detach().double()
        assert got.shape == ref.shape and got.dim() == 2, (what, got.shape, ref.shape)
        if not bool(torch.isfinite(got).all()):
            self.missed.append(f"{what}: non-finite rows [{key}]")
            return
        nrm, err = ref.norm(dim=1), (got - ref).norm(dim=1)
        live = nrm >= 1e-3 * nrm.mean() if own else torch.zeros_like(nrm, dtype=torch.bool)
        dead = int((~live).sum())
        if own and not dead <= 0.01 * ref.shape[0]:
            self.missed.append(f"{what}: {dead} of {ref.shape[0]} rows without reference norm [{key}]")
        if dead:
            i = int(err[~live].argmax())
            self.bar(float(err[~live][i] / nrm.mean()), limit, f"{what} (row {int((~live).nonzero()[i])} of {ref.shape[0]}, against the mean norm)", key, cap=UNIT_GRAD)
        if dead < ref.shape[0]:
            e = (err / nrm.clamp_min(1e-30))[live]
            i = int(e.argmax())
            self.bar(float(e[i]), limit, f"{what} (row {int(live.nonzero()[i])} of {ref.shape[0]})", key, cap=UNIT_GRAD)

    def done(self):
        print(f"\n{self.case}: worst value / bar")
        for k, (v, lim, what) in sorted(self.worst.items()):
            print(f"    {k:28s} {v:.2e} / {'unset' if lim is None else format(lim, '.1e')}   ({what})")
        assert not self.missed, f"{self.case}: {len(self.missed)} misses:\n" + "\n".join(self.missed[:40])


def unit_meshgrid(H, W):
    ys, xs = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    return torch.stack([xs, ys])


def make_model(case, dev, tmp):
    from py4cast_amd.graphlam import GraphLamMI355X, GraphLamSettings
    from py4cast_amd.hilam import HiLamMI355X, HiLamSettings
    from py4cast_amd.hilamparallel import HiLamParallelMI355X, HiLamParallelSettings

    name, hw, key, aggr, layers, (cin, cout) = CASES[case]
    if hw is None:
        hw, _ = N.smallest_grid_past_caps_of(name, *BENCH, cus_of(dev), processor_layers=layers)
    kls, skls = {"graphlam": (GraphLamMI355X, GraphLamSettings), "hilam": (HiLamMI355X, HiLamSettings),
                 "hilampar": (HiLamParallelMI355X, HiLamParallelSettings)}[name]
    kw = dict(tmp_dir=str(tmp), activation_dtype=key, processor_layers=layers)
    if name == "graphlam":
        kw["mesh_aggr"] = aggr
    st = skls(**kw)
    kls.rank_zero_setup(st, unit_meshgrid(*hw))
    torch.manual_seed(51)
    m = kls(cin, cout, hw, st).to(dev)
    g = torch.Generator().manual_seed(52)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith(("3.weight", "3.bias")):      # LayerNorm affine off its initial 1 / 0 by +-(0.1 ... 0.3): a dropped gamma / beta shows
                d = (0.1 + 0.2 * torch.rand(p.shape, generator=g)) * (1 - 2 * (torch.rand(p.shape, generator=g) < 0.5).float())
                p.add_(d.to(dev))
    gd = torch.Generator(device=dev).manual_seed(53)
    x = torch.randn(2, hw[0] * hw[1], cin, device=dev, generator=gd)
    dy = torch.randn(2, hw[0] * hw[1], cout, device=dev, generator=gd)
    return m, x, dy, hw


def step(m, x, dy):
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), xg.grad


@pytest.fixture(scope="module", params=list(CASES))
def run(request, gpu_device, tmp_path_factory):
    torch.cuda.empty_cache()
    case = request.param
    m, x, dy, hw = make_model(case, gpu_device, tmp_path_factory.mktemp("graphs"))
    bf = CASES[case][2] == "bf16"
    if bf:                                   # the benchmark's route: gradient buffers exist
        for p in m.parameters():
            p.grad = torch.zeros_like(p)
    with N.Recorder(m, cus_of(gpu_device)) as rec:
        y, dx = step(m, x, dy)
    for n in rec.nodes:
        assert n.outs and any(o is not None for o in n.outs), f"{n.kind} {n.name}: no output recorded"
        assert any(d is not None for d in n.dys), f"{n.kind} {n.name}: no incoming gradient recorded"
    g_run = {name: p.grad.detach().clone() for name, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    yield SimpleNamespace(case=case, name=CASES[case][0], model=m, x=x, dy=dy, y=y, dx=dx, rec=rec, g_run=g_run, hw=hw, bf16=bf, buffers=bf,
                          layers=CASES[case][4], cus=cus_of(gpu_device), replays={})
    del m, rec, g_run
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ replay
def fresh(t):
    if t is None or not isinstance(t, torch.Tensor):
        return t
    return t.detach().clone().requires_grad_(True) if t.is_floating_point() else t


class Leaves:
    """fresh leaves of a node's operands: a parameter operand becomes the matching view of a fresh clone of the whole parameter (with a
    zero-filled gradient buffer where the case has buffers), shared by the node's operands that are views of the same parameter"""

    def __init__(self, run):
        self.run, self.params = run, {}

    def of(self, v):
        if isinstance(v, list):
            return [self.of(u) for u in v]
        if isinstance(v, tuple) and v and v[0] == "param":
            _, name, shape, stride, off = v
            if name not in self.params:
                q = self.run.model.get_parameter(name).detach().clone().requires_grad_(True)
                if self.run.buffers:
                    q.grad = torch.zeros_like(q)
                self.params[name] = q
            q = self.params[name]
            whole = tuple(q.shape) == shape and tuple(q.stride()) == stride and off == 0
            return q if whole else q.as_strided(shape, stride, q.storage_offset() + off)
        return fresh(v)

    def grad(self, v):
        """the gradient of a parameter operand: its region of the fresh parameter's .grad"""
        _, name, shape, stride, off = v
        g = self.params[name].grad        # (autograd may have taken a view of a larger buffer for it: the offset counts from ITS start)
        return None if g is None else g.as_strided(shape, stride, g.storage_offset() + off)


def backward(outs, dys):
    pairs = [(o, d.clone()) for o, d in zip(outs, dys) if o is not None and d is not None and o.requires_grad]
    torch.autograd.backward([o for o, _ in pairs], [d for _, d in pairs])
    torch.cuda.synchronize()


def _replay(run, node):
    from py4cast_amd import graphlam as GL
    from py4cast_amd import hilamparallel as HP
    from py4cast_amd import ops_graph as G
    from py4cast_amd import ops_mlp as M
    from py4cast_amd import ops_nodeproj as NP
    from py4cast_amd import ops_rows as R

    a, k, o = node.args, node.kind, node.opts
    if k in ("mlp", "inet", "edge_messages", "node_update"):
        mod = node.module
        ps = dict(mod.named_parameters())
        for p in ps.values():
            p.grad = torch.zeros_like(p) if run.buffers else None
        ins = {s: fresh(t) for s, t in a.items()}
        if k == "mlp":
            outs = GL._run(mod, ins["x"], ins["x"] if o["res_is_x"] else ins["res"], o["keep_pad"])
        elif k == "inet":
            outs = GL.InteractionNet.forward(mod, ins["rec"] if o["same"] else ins["send"], ins["rec"], ins["edge"], o["edges"])
        elif k == "edge_messages":
            outs = HP._edge_messages(mod, ins["rec"] if o["same"] else ins["send"], ins["rec"], ins["edge"], o["edges"])
        else:
            outs = HP._node_update(mod, ins["rec"], ins["agg"])
        outs = outs if isinstance(outs, tuple) else (outs,)
        backward(outs, node.dys)
        grads = {s: (t.grad if isinstance(t, torch.Tensor) and t.requires_grad else None) for s, t in ins.items()}
        grads.update({n: (None if p.grad is None else p.grad.clone()) for n, p in ps.items()})
        for p in ps.values():
            p.grad = None
        return SimpleNamespace(outs=[None if t is None else t.detach() for t in outs], grads=grads)
    L = Leaves(run)
    ins = {s: L.of(v) for s, v in a.items()}
    if k == "row_mlp":
        res = ins["x"] if o["res_is_x"] else ins["res"]
        outs = M.row_mlp(ins["x"], ins["w1"], ins["b1"], ins["w2"], ins["b2"], ins["gamma"], ins["beta"], o["eps"], ins["ga"], ins["gb"], o["edges"],
                         res, o["want_out"], o["grads_in_place"])
    elif k == "node_proj":
        outs = NP.node_proj(ins["x"], ins["weights"], o["grads_in_place"], o["passthrough"])
        assert o["native"] == (type(outs[0].grad_fn).__name__ == "_NodeProjBackward"), f"{node.name}: replayed on another route"
        if o["passthrough"] and not o["native"]:
            outs = outs[:-1] + (None,)            # (the fallback hands x itself back: no output of the node)
    elif k == "segment_sum":
        outs = G.aggregate_sum(ins["msg"], o["edges"])
    elif k == "gather_add":
        outs = G.edge_gather_add(ins["base"], ins["a"], ins["b"], o["edges"], o["act"])
    elif k == "ln":
        outs = R.row_layer_norm(ins["x"], ins["g"], ins["b"], o["eps"], ins["res"])
    elif k == "linear":
        outs = R.row_linear(ins["x"], ins["w"], ins["b"], o["grads_in_place"])
    else:
        outs = torch.nn.functional.linear(ins["x"], ins["w"], ins["b"])
    outs = outs if isinstance(outs, tuple) else (outs,)
    backward(outs, node.dys)
    grads = {}
    for s, v in a.items():
        vs, ts = (v, ins[s]) if isinstance(v, list) else ([v], [ins[s]])
        for j, (u, t) in enumerate(zip(vs, ts)):
            key = f"{s}{j}" if isinstance(v, list) else s
            if isinstance(u, tuple) and u and u[0] == "param":
                grads[key] = L.grad(u)
            elif isinstance(t, torch.Tensor) and t.requires_grad:
                grads[key] = t.grad
    return SimpleNamespace(outs=[None if t is None else t.detach() for t in outs], grads=grads)


def replay(run, node):
    if node.index not in run.replays:
        run.replays[node.index] = _replay(run, node)
    return run.replays[node.index]


def from_library(run, node):
    """the node, or for a composed node one of the nodes inside it, runs a library GEMM (no bit-for-bit promise)"""
    if node.kind == "flinear":
        return True
    return any(n.kind == "flinear" for n in run.rec.nodes if _inside(run.rec, n, node))


def _inside(rec, n, node):
    while n.parent is not None:
        if n.parent == node.index:
            return True
        n = rec.nodes[n.parent]
    return False


def test_replay_is_bit_identical(run):
    exempt = []
    for node in run.rec.nodes:
        r = replay(run, node)
        what = f"{node.kind} {node.name}"
        lib = from_library(run, node)
        assert not (lib and run.bf16), f"{what}: a library GEMM in the bf16 flavour (graphlam.py: every kernel is native)"
        for j, want in enumerate(node.outs):
            if want is None:
                continue
            if lib:
                assert rel(r.outs[j], want) <= 1e-5, f"{what}: replayed output {j} {rel(r.outs[j], want):.2e} off the in-network one"
            else:
                same(r.outs[j], want, f"{what} out {j}")
        if lib:
            exempt.append(what)
            continue
        again = _replay(run, node)
        for s, g in r.grads.items():
            if g is not None or again.grads[s] is not None:
                same(again.grads[s], g, f"{what} d{s}, replayed twice")
    print(f"\n{run.case}: {len(run.rec.nodes)} nodes replayed; exempt from bit-identity (library GEMMs): {exempt}")
    assert run.bf16 or all(w.startswith(("flinear", "mlp", "inet")) for w in exempt)


# ------------------------------------------------------------------------------------------------ launch table
def test_launch_table(run):
    """every leaf's recorded sizes give the launches gnn_nodes.launch_table derives from the grid alone; the caps cases run inside the
    loops the benchmark runs inside"""
    if not run.bf16:
        assert not run.rec.of("row_mlp", "node_proj"), "the fp32 flavour on a fused kernel"
        return
    got = {n.name: n.launches for n in run.rec.leaves()}
    want = N.launch_table(run.name, 2, *run.hw, run.cus, processor_layers=run.layers)
    assert got.keys() == want.keys(), sorted(set(got) ^ set(want))
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert all(n.opts["native"] for n in run.rec.of("node_proj")), "a node projection off its own kernels"
    bench = N.launch_table(run.name, *BENCH, run.cus, processor_layers=run.layers)
    looping = sorted({l.kernel for ls in want.values() for l in ls if l.capped})
    if run.case.endswith("caps-bf16"):
        grid, table = N.smallest_grid_past_caps_of(run.name, *BENCH, run.cus, processor_layers=run.layers)
        assert grid == run.hw and table == bench and grid[0] * grid[1] < BENCH[1] * BENCH[2]
        assert N.loop_signature(want) == N.loop_signature(bench)
        assert set(looping) >= {"row_mlp_fwd", "row_mlp_bwd", "segment_sum", "edge_gather_add_fwd", "node_proj_fwd", "node_proj_dgrad", "node_proj_wgrad"}
        print(f"\n{run.case}: grid {grid}, {run.cus} CUs; kernels that loop past their cap: {looping}")
        for name in sorted(bench):
            print(f"    {name:40s} " + "  ".join(f"{l.kernel}: {l.passes}{'*' if l.capped else ''}"
                                                 + (f" s{l.split_log2}" if l.split_log2 is not None else "") + (f" [{l.slots}]" if l.slots else "")
                                                 for l in bench[name]))
    else:
        # (36 x 45 stays below every cap; at 81 x 96 only the backward of the edge MLP over the 2 x 21 k grid-to-mesh edges passes its own)
        assert not looping or (run.hw == (81, 96) and looping == ["row_mlp_bwd"]), f"{run.case}: a toy case past a cap: {looping}"
        shared = set(want) & set(bench)
        assert N.loop_signature({k: want[k] for k in shared}) != N.loop_signature({k: bench[k] for k in shared}), "the toy grid has the benchmark's table"


# ------------------------------------------------------------------------------------------------ float64
def weights64(node, run, *slots):
    return [None if node.args[s] is None else N.gemm_w(tensor_of(run, node.args[s]), run.bf16) for s in slots]


def tensor_of(run, v):
    """the recorded operand as a tensor (a parameter operand: the live parameter's view)"""
    if isinstance(v, tuple) and v and v[0] == "param":
        _, name, shape, stride, off = v
        p = run.model.get_parameter(name).detach()
        return p.as_strided(shape, stride, p.storage_offset() + off)
    return v


def module_leaves(mod, rounded):
    """float64 leaves of a module's parameters as its kernels read them (Linear weights bf16-rounded when `rounded`)"""
    return {n: (N.gemm_w(p, rounded) if n.endswith(("0.weight", "2.weight")) else p.detach().double()).requires_grad_(True)
            for n, p in mod.named_parameters()}


def test_nodes_against_float64(run):
    bf = run.bf16
    T = Tally(run.case)
    bar = T.bar

    def near(got, ref, what, grad=False, rows=None):
        """an activation-typed map: the bf16-map bars, or the fp32 flavour's output / gradient bar"""
        got, ref = got.detach().double(), ref.detach().double()
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        if bf:
            bar(float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)), 6e-3, f"{what} (max)", "bf16 map, max")
            bar(rel(got, ref), 3e-3, f"{what} (2-norm)", "bf16 map, 2-norm")
        else:
            bar(rel(got, ref), 1e-4 if grad else 1e-5, what, "fp32 grad" if grad else "fp32 out")
        if rows:
            T.rows(got, ref, what, rows if bf else "fp32 rows", ROW_BARS[rows if bf else "fp32 rows"], own=not grad)

    def composed(v, key, what, out):
        if bf:
            bar(v, COMPOSED_BARS[key], what, key, cap=UNIT_OUT if out else UNIT_GRAD)
        else:
            bar(v, 1e-5 if out else 1e-4, what, "fp32 composed " + ("out" if out else "grad"))

    def wgrad(got, ref, what, limit=5e-4, key="GEMM dW"):
        bar(rel(got, ref), limit if bf else 1e-4, what, key if bf else "fp32 grad")

    for node in run.rec.nodes:
        r = replay(run, node)
        a, o, k, g = node.args, node.opts, node.kind, r.grads
        what = f"{k} {node.name}"
        if k == "row_mlp":
            e = o["edges"]
            ia, ib = (None, None) if e is None else (e.src, e.dst)
            w1, w2 = weights64(node, run, "w1", "w2")
            b1, b2, gm, bt = (tensor_of(run, a[s]) for s in ("b1", "b2", "gamma", "beta"))
            fold_res = o["res_is_x"]

            def fn(x, w1_, b1_, w2_, b2_, gm_, bt_, ga, gb, res):
                return N.row_mlp(x, w1_, b1_, w2_, b2_, gm_, bt_, o["eps"], ga, ia, gb, ib, x if fold_res else res, round_hidden=bf)

            (y64, yr64), gr = N.node(fn, (a["x"], w1, b1, w2, b2, gm, bt, a["ga"], a["gb"], None if fold_res else a["res"]), node.dys)
            O = w2.shape[0]
            for j, ref in enumerate((y64, yr64)):
                if node.outs[j] is not None:
                    got = r.outs[j][:, :O]
                    base = a["x"].double() if (j == 1 and fold_res) else (a["res"].double() if j == 1 else 0)
                    composed(rel(got.double() - base, ref - base), "row_mlp y", f"{what} {'y + res' if j else 'y'}", True)
                    T.rows(got.double() - base, ref - base, f"{what} {'y + res' if j else 'y'}", "row_mlp rows", ROW_BARS["row_mlp rows"])
                    assert not r.outs[j][:, O:].any(), f"{what}: padding features of the output are not zero"
            if g.get("x") is not None:
                base = node.dys[1].double() if (fold_res and node.dys[1] is not None) else 0      # (res is x: the kernel stores dx + dy_res)
                composed(rel(g["x"].double() - base, gr[0] - base), "row_mlp dx", f"{what} dx", False)
                T.rows(g["x"].double() - base, gr[0] - base, f"{what} dx", "row_mlp grad rows", ROW_BARS["row_mlp grad rows"], own=False)
            for s, ref in (("w1", gr[1]), ("w2", gr[3])):
                composed(rel(g[s], ref), "row_mlp dW", f"{what} d{s}", False)
            for s, ref in (("b1", gr[2]), ("b2", gr[4]), ("gamma", gr[5]), ("beta", gr[6])):
                if ref is not None:
                    composed(rel(g[s], ref), "row_mlp db", f"{what} d{s}", False)
            for s, ref in (("ga", gr[7]), ("gb", gr[8])):
                if ref is not None and g.get(s) is not None:
                    composed(rel(g[s], ref), "row_mlp daddend", f"{what} d{s}", False)
                    T.rows(g[s], ref, f"{what} d{s}", "row_mlp grad rows", ROW_BARS["row_mlp grad rows"], own=False)
            if a["res"] is not None and not fold_res:
                same(g["res"], node.dys[1], f"{what} dres")
        elif k == "node_proj":
            ws = [N.gemm_w(tensor_of(run, w), bf) for w in a["weights"]]
            n = len(ws)
            ys, gr = N.node(lambda x, *w: N.node_proj(x, w, o["passthrough"] and o["native"]), (a["x"], *ws), node.dys)
            for j in range(n):
                near(r.outs[j], ys[j], f"{what} y{j}", rows="node_proj rows")
                wgrad(g[f"weights{j}"], gr[1 + j], f"{what} dW{j}")
            near(g["x"], gr[0], f"{what} dx", grad=True, rows="node_proj grad rows")
            if o["passthrough"] and o["native"]:
                same(r.outs[n], a["x"], f"{what}: the passthrough tensor")
        elif k == "segment_sum":
            e = o["edges"]
            y64, (dm64,) = N.node(lambda m: N.segment_sum(m, e.dst, e.n_dst), (a["msg"],), node.dy)
            near(r.outs[0], y64, f"{what} sum", rows="single-kernel rows")
            same(g["msg"], N.rows_of(node.dy, e.dst), f"{what}: the adjoint gather")
            assert rel(dm64, N.rows_of(node.dy, e.dst)) == 0
        elif k == "gather_add":
            e = o["edges"]
            y64, gr = N.node(lambda b_, a_, c_: N.edge_gather_add(b_, a_, e.src, c_, e.dst, o["act"]), (a["base"], a["a"], a["b"]), node.dy)
            near(r.outs[0], y64, f"{what} y", rows="fp32 rows")
            for s, ref in zip(("base", "a", "b"), gr):
                if ref is not None:
                    near(g[s], ref, f"{what} d{s}", grad=True)
        elif k == "ln":
            gm, bt = tensor_of(run, a["g"]), tensor_of(run, a["b"])
            y64, gr = N.node(lambda x, g_, b_, res: N.ln_res(x, g_, b_, o["eps"], res), (a["x"], gm, bt, a["res"]), node.dy)
            near(r.outs[0], y64, f"{what} y", rows="fp32 rows")
            near(g["x"], gr[0], f"{what} dx", grad=True)
            for s, ref in (("g", gr[1]), ("b", gr[2])):
                bar(rel(g[s], ref), 2e-3 if bf else 1e-4, f"{what} d{s}", "LayerNorm dgamma, dbeta" if bf else "fp32 grad")
            if a["res"] is not None:
                same(g["res"], node.dy, f"{what} dres")
        elif k in ("linear", "flinear"):
            w = N.gemm_w(tensor_of(run, a["w"]), bf)
            y64, gr = N.node(N.linear, (a["x"], w, tensor_of(run, a["b"])), node.dy)
            near(r.outs[0], y64, f"{what} y", rows="fp32 rows")
            if g.get("x") is not None:
                near(g["x"], gr[0], f"{what} dx", grad=True)
            wgrad(g["w"], gr[1], f"{what} dW")
            if a["b"] is not None:
                wgrad(g["b"], gr[2], f"{what} db")
        else:
            mod = node.module
            P = module_leaves(mod, bf)
            names = list(P)
            tens = {s: (None if t is None else t.double().requires_grad_(True)) for s, t in a.items()}
            with torch.enable_grad():
                if k == "mlp":
                    x = tens["x"]
                    if "0.weight" not in P:      # edge_mlp[2:] of the fp32 flavour (a slice keeps the layers' names): Linear - LayerNorm
                        yr = N.ln_res(N.linear(x, P["2.weight"], P["2.bias"]), P["3.weight"], P["3.bias"], res=tens["res"])
                    else:
                        yr = N.mlp_rows(x, P, "", layer_norm="3.weight" in P, res=x if o["res_is_x"] else tens["res"], round_hidden=bf)
                    refs, key = (yr,), "mlp"
                elif k == "node_update":
                    rec_, agg = tens["rec"], tens["agg"]
                    refs, key = (rec_ + N.mlp_rows(torch.cat([rec_, agg], dim=-1), P, "", round_hidden=bf),), "inet"
                else:
                    e = o["edges"]
                    rec_ = tens["rec"]
                    send = rec_ if o["same"] else tens["send"]
                    if k == "inet":
                        refs = N.interaction_net(send, rec_, tens["edge"], e.src, e.dst, P, "", mod.update_edges, mod.aggr, round_hidden=bf)
                        refs = refs if isinstance(refs, tuple) else (refs,)
                    else:
                        msg = N.mlp_rows(torch.cat([tens["edge"], N.rows_of(send, e.src), N.rows_of(rec_, e.dst)], dim=-1), P, "", round_hidden=bf)
                        refs = (msg, tens["edge"] + msg)
                    key = "inet"
                live = [(s, t) for s, t in tens.items() if t is not None and not (s == "send" and o.get("same")) and not (s == "res" and o.get("res_is_x"))]
                pairs = [(y, d.double()[:, :y.shape[1]]) for y, d in zip(refs, node.dys) if d is not None]
                gr = torch.autograd.grad([y for y, _ in pairs], [t for _, t in live] + [P[n] for n in names], [d for _, d in pairs], allow_unused=True)
            for j, ref in enumerate(refs):
                if node.outs[j] is not None:
                    got = r.outs[j][:, :ref.shape[1]]
                    composed(rel(got, ref), f"{key} y", f"{what} out {j}", True)
                    T.rows(got, ref.detach(), f"{what} out {j}", "composed rows" if bf else "fp32 rows", ROW_BARS["composed rows" if bf else "fp32 rows"])
            for (s, _), ref in zip(live, gr):
                if ref is not None and g.get(s) is not None:
                    composed(rel(g[s], ref), f"{key} dx", f"{what} d{s}", False)
            for n, ref in zip(names, gr[len(live):]):
                assert g[n] is not None and ref is not None, f"{what}: {n} got no gradient"
                composed(rel(g[n], ref), f"{key} dparam", f"{what} d{n}", False)
    T.done()


# ------------------------------------------------------------------------------------------------ wiring
def orders(terms, dtype):
    """the sums of `terms` in every order autograd may have accumulated them (left to right over a permutation), in the tensor's dtype"""
    if len(terms) <= 2:
        yield sum(terms[1:], terms[0]).to(dtype)
        return
    for perm in itertools.permutations(range(len(terms))):
        if perm[0] > perm[1]:
            continue                       # (a + b = b + a)
        t = terms[perm[0]]
        for i in perm[1:]:
            t = t + terms[i]
        yield t.to(dtype)


def edge(run, got, terms, what, producers):
    assert got is not None and terms, f"{what}: missing"
    terms = [t.reshape(got.shape) for t in terms]
    if any(from_library(run, p) for p in producers):
        lim = 1e-5
        best = min(rel(got, t) for t in orders(terms, got.dtype))
        assert best <= lim, f"{what}: {best:.2e} > {lim:.0e} (a library GEMM among the producers)"
        return
    if not any(torch.equal(got, t) for t in orders(terms, got.dtype)):
        best = min(rel(got, t) for t in orders(terms, got.dtype))
        raise AssertionError(f"{what}: the gradient received is no ordering of its {len(terms)} terms (closest {best:.2e})")


def test_wiring_is_bit_identical(run):
    rec, m = run.rec, run.model
    leaves = rec.leaves()
    consumers = {}            # (leaf index, slot) -> [(consumer leaf, operand key)]
    for c in leaves:
        for key, srcv in c.src_leaf.items():
            if key == "res" and c.opts.get("res_is_x"):
                continue                                   # (the folded dx + dy_res arrives under "x")
            consumers.setdefault(srcv, []).append((c, key))
    checked, loose = 0, []
    # (the fp32 flavour joins its library calls with torch arithmetic -- cat, +, the activation -- that the recorder does not see: its
    #  tensors have consumers beside the recorded ones, and autograd's own sums are not this project's code)
    for p in (leaves if run.bf16 else []):
        for j, out in enumerate(p.outs):
            if out is None or p.dys[j] is None:
                continue
            cons = consumers.get((p.index, j), [])
            if not cons:
                loose.append((p, j))
                continue
            if len(cons) > 6:
                continue
            terms = [replay(run, c).grads[key] for c, key in cons]
            assert all(t is not None for t in terms), f"{p.name} out {j}: a consumer gave no gradient: {[(c.name, k) for c, k in cons]}"
            edge(run, p.dys[j], terms, f"{p.kind} {p.name} out {j} <- " + " + ".join(f"{c.name}.{k}" for c, k in cons), [c for c, _ in cons])
            checked += 1
    # outputs no recorded leaf consumes directly: they pass through torch glue, checked piece by piece
    B = run.x.shape[0]
    by_shape = {}
    for c in leaves:
        for key, v in c.args.items():
            if isinstance(v, torch.Tensor) and v.is_floating_point() and key not in c.src_leaf and v.dim() == 2:
                by_shape.setdefault(v.shape[0], []).append((c, key, v))
    unexplained = []
    for p, j in loose:
        out = p.outs[j]
        if p.name == "output_map":                           # -> the network's output: its dy is the network's, zero in the padding features
            O = run.dy.shape[-1]
            same(p.dys[j][:, :O].contiguous(), run.dy.reshape(-1, O).to(out.dtype), "output_map: the network's dy")
            assert not p.dys[j][:, O:].any(), "output_map: the padding features took a gradient"
            continue
        # a static embedding: expanded over the batch; its gradient is the sum over the batch of its consumers' (two terms per consumer)
        rep = out.unsqueeze(0).expand(B, *out.shape).reshape(B * out.shape[0], -1)
        cons = [(c, key) for c, key, v in by_shape.get(B * out.shape[0], []) if v.shape == rep.shape and torch.equal(v, rep)
                and not (key == "res" and c.opts.get("res_is_x"))]
        if cons:
            terms = [replay(run, c).grads[key].reshape(B, *out.shape).float().sum(0).to(out.dtype) for c, key in cons]
            edge(run, p.dys[j], terms, f"static embedding {p.name} <- sum over the batch of " + " + ".join(f"{c.name}.{k}" for c, k in cons),
                 [c for c, _ in cons])
            checked += 1
            continue
        unexplained.append(f"{p.kind} {p.name} out {j}")
    # what remains passes through torch arithmetic the recorder does not see: the mean aggregation's division (segment sums of a mean
    # processor), HiLAMParallel's sum of the edge sets' aggregates per level, and in the fp32 flavour the torch glue between library calls
    if run.bf16:
        ok = (lambda s: ".aggregate" in s) if (run.name == "hilampar" or "mean" in run.case) else (lambda s: False)
        assert all(ok(s) for s in unexplained), f"outputs whose gradient no consumer explains: {unexplained}"
    # the network's dx is the grid embedder's (through the cast to the activation type)
    first = rec["grid_embedder"] if run.bf16 else rec["grid_embedder.0.flinear"]
    gx = replay(run, first).grads["x"]
    if run.bf16:
        same(gx.to(run.dx.dtype).reshape(run.dx.shape), run.dx, "the network's dx")
    else:
        assert rel(gx.reshape(run.dx.shape), run.dx) <= 1e-5
    # every p.grad is the leaf replays'; every parameter (or column block of it) belongs to exactly one leaf
    owned = {}
    for node in leaves:
        r = replay(run, node)
        for s, v in node.args.items():
            for i, u in enumerate(v if isinstance(v, list) else [v]):
                if not (isinstance(u, tuple) and u and u[0] == "param"):
                    continue
                key = f"{s}{i}" if isinstance(v, list) else s
                _, pname, shape, stride, off = u
                region = (off, shape)
                for other, who in owned.setdefault(pname, {}).items():
                    lo, hi = sorted((other, region))
                    assert lo[0] + lo[1][-1] <= hi[0], f"{pname}: {node.name}.{key} overlaps {who}"
                owned[pname][region] = f"{node.name}.{key}"
                got = r.grads[key]
                assert got is not None, f"{node.name}.{key}: no gradient for {pname}"
                want = run.g_run[pname].as_strided(shape, stride, off)
                if from_library(run, node):
                    assert rel(got, want) <= 1e-5, f"{node.name}.{key}: p.grad of {pname} {rel(got, want):.2e}"
                else:
                    same(got.contiguous(), want.contiguous(), f"{node.name}.{key}: p.grad of {pname}")
    names = [n for n, _ in m.named_parameters()]
    assert sorted(owned) == sorted(names), sorted(set(names) ^ set(owned))
    for n, p in m.named_parameters():
        cols = sum(shape[-1] for _, shape in owned[n])
        assert cols == p.shape[-1], f"{n}: {cols} of {p.shape[-1]} columns owned: {owned[n]}"
        if n.endswith("edge_mlp.0.weight") or ".edge_mlps." in n and n.endswith(".0.weight"):
            assert sorted(off for off, _ in owned[n]) == ([0, 64, 128] if run.bf16 else [0, 64, 128]), (n, owned[n])
        if n.endswith("aggr_mlp.0.weight") or ".aggr_mlps." in n and n.endswith(".0.weight"):
            assert sorted(off for off, _ in owned[n]) == ([0, 64] if run.bf16 else [0]), (n, owned[n])
    # composed nodes: their parameter gradients are the leaf nodes'
    for comp in rec.of("mlp", "inet", "edge_messages", "node_update"):
        pre = rec.names.get(id(comp.module))
        if pre is None or from_library(run, comp):
            continue
        for n, _ in comp.module.named_parameters():
            same(replay(run, comp).grads[n], run.g_run[f"{pre}.{n}"], f"{comp.name}: {n} of the composed replay")
    counts = (len(rec.nodes), len(leaves), len(names))
    print(f"\n{run.case}: {counts[0]} nodes ({counts[1]} leaves: " + ", ".join(f"{len(rec.of(k))} {k}" for k in N.KINDS if rec.of(k))
          + f"), {counts[2]} parameters, {checked} edges checked, {len(unexplained)} through torch glue")
    assert counts == COUNTS[run.case], (counts, COUNTS[run.case])
    assert checked >= len(leaves) // 2 or not run.bf16


# ------------------------------------------------------------------------------------------------ sink route
def test_sink_route_adds_into_grad(run):
    from py4cast_amd import _lib as L
    from py4cast_amd import graphlam as GL
    from py4cast_amd.trainer import FlatDDP

    if run.case not in ("graphlam-toy-bf16", "graphlam-toy-mean-bf16", "hilam-3lev-bf16", "hilampar-3lev-bf16"):
        return
    assert GL.GRADS_IN_PLACE
    m = run.model
    m.zero_grad(set_to_none=True)
    step(m, run.x, run.dy)                                       # the `.grad is None` run: node_proj on its row_linear fallback
    worst = max((rel(p.grad, run.g_run[n]), n) for n, p in m.named_parameters())
    print(f"\n{run.case}: .grad is None against zero-filled buffers, worst parameter {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= UNIT_GRAD, worst
    g = torch.Generator(device=run.x.device).manual_seed(11)
    prefill = {n: (torch.rand(p.shape, device=p.device, generator=g) + 0.5) * (1 - 2 * (torch.rand(p.shape, device=p.device, generator=g) < 0.5))
               for n, p in m.named_parameters()}
    for n, p in m.named_parameters():
        p.grad = prefill[n].clone()
    step(m, run.x, run.dy)
    assert L.lib().p4c_grad_reduce_pending() == 0
    for n, p in m.named_parameters():
        same(p.grad, prefill[n] + run.g_run[n], f"prefilled .grad: {n}")
    ddp = FlatDDP(m, 1)
    ddp.flat_grad.fill_(3.0)
    for n, p in m.named_parameters():
        assert p.grad.data_ptr() >= ddp.flat_grad.data_ptr(), n
        p.grad.copy_(prefill[n])
    step(m, run.x, run.dy)
    assert L.lib().p4c_grad_reduce_pending() == 0, "the deferred reduction queue is not empty after the backward"
    for n, p in m.named_parameters():
        same(p.grad, prefill[n] + run.g_run[n], f"FlatDDP .grad: {n}")
    m.zero_grad(set_to_none=True)


# ------------------------------------------------------------------------------------------------ direct kernel cases past each cap
def _bf(t):
    return t.to(torch.bfloat16)


def _edges(E, n_src, n_dst, dev, gen, hub=0.0, empty=False):
    """E random edges; `hub`: that share of them go to one receiver; `empty`: every 7th receiver (and the last) gets none"""
    from py4cast_amd.ops_graph import EdgeSet

    src = torch.randint(0, n_src, (E,), device=dev, generator=gen)
    dst = torch.randint(0, n_dst, (E,), device=dev, generator=gen)
    if empty:
        dst = torch.where((dst % 7 == 3) | (dst == n_dst - 1), (dst + 1) % (n_dst - 1), dst)
    if hub:
        dst[torch.randperm(E, device=dev, generator=gen)[:int(hub * E)]] = n_dst // 3 - (n_dst // 3) % 7
    return EdgeSet(src, dst, n_src, n_dst)


MLP_CONFIGS = {            # K real, outputs, LayerNorm, addends (None / "edges" / "rows"), res (None / "x" / "other"), gradient buffers
    "k16": (16, 64, True, None, None, False),
    "k64-gather-res-is-x-sink": (64, 64, True, "edges", "x", True),
    "k64-gather-res": (64, 64, True, "edges", "other", False),
    "k69-res-sink": (69, 64, True, None, "other", True),
    "k64-out60": (64, 60, False, None, None, False),
    "k64-aligned-addend-res-sink": (64, 64, True, "rows", "other", True),
}


@pytest.mark.parametrize("config", list(MLP_CONFIGS))
@pytest.mark.parametrize("size", ["bwd-cap", "fwd-cap"])
def test_row_mlp_past_the_caps(gpu_device, size, config):
    """the fused row MLP where a wave loops over several tiles: R = 128 x CUs x 2 + 17 (the backward's waves take three tiles, the forward's
    one) and R = 512 x CUs + 33 (the forward loops too); odd tails, so the last tile is partial and the last workgroup has idle waves"""
    from py4cast_amd.ops_mlp import row_mlp

    dev, cus = gpu_device, cus_of(gpu_device)
    R = 128 * cus * 2 + 17 if size == "bwd-cap" else 512 * cus + 33
    assert N.mlp_launch(R, 1, cus, bwd=True).capped and N.mlp_launch(R, 4, cus).capped == (size == "fwd-cap") and R % 32
    K, O, ln, addends, res_kind, buffers = MLP_CONFIGS[config]
    gen = torch.Generator(device=dev).manual_seed(61)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    x = _bf(rn(R, K)).requires_grad_(True)
    ps = dict(w1=rn(64, K) * K ** -0.5, b1=rn(64) * 0.1, w2=rn(O, 64) * 0.125, b2=rn(O) * 0.1)
    if ln:
        ps.update(gamma=1 + 0.3 * rn(64).clamp(-1, 1), beta=0.3 * rn(64).clamp(-1, 1))
    ps = {k: v.requires_grad_(True) for k, v in ps.items()}
    if buffers:
        for p in ps.values():
            p.grad = torch.full_like(p, 0.5)
    edges = ga = gb = None
    if addends == "edges":
        ns, nr = R // 3 + 1, R // 29 + 1
        edges = _edges(R, ns, nr, dev, gen)
        ga, gb = _bf(rn(ns, 64)).requires_grad_(True), _bf(rn(nr, 64)).requires_grad_(True)
    elif addends == "rows":
        ga = _bf(rn(R, 64)).requires_grad_(True)
    other = _bf(rn(R, 64)).requires_grad_(True) if res_kind == "other" else None
    res = x if res_kind == "x" else other
    dy, dyr = _bf(rn(R, 64)), _bf(rn(R, 64))
    if O < 64:
        dy[:, O:] = 0

    def once():
        for t in (x, ga, gb, other):
            if t is not None:
                t.grad = None
        y, yr = row_mlp(x, ps["w1"], ps["b1"], ps["w2"], ps["b2"], ps.get("gamma"), ps.get("beta"), 1e-5, ga, gb, edges, res, True, buffers)
        backward((y, yr), (dy, dyr if res is not None else None))
        pg = {k: (p.grad - 0.5 if buffers else p.grad).clone() for k, p in ps.items()}
        for p in ps.values():
            p.grad = torch.full_like(p, 0.5) if buffers else None
        return (y.detach(), None if yr is None else yr.detach()), {k: (None if t is None else t.grad.clone()) for k, t in
                                                                   (("x", x), ("ga", ga), ("gb", gb), ("res", other))}, pg

    (y, yr), gi, pg = once()
    (y2, yr2), gi2, pg2 = once()
    same(y2, y, "row_mlp y, twice")
    for k in gi:
        if gi[k] is not None:
            same(gi2[k], gi[k], f"row_mlp d{k}, twice")
    for k in pg:
        same(pg2[k], pg[k], f"row_mlp d{k}, twice")
    ia, ib = (None, None) if edges is None else (edges.src, edges.dst)
    fold = res_kind == "x"

    def fn(x_, w1, b1, w2, b2, gm, bt, ga_, gb_, res_):
        return N.row_mlp(x_, w1, b1, w2, b2, gm, bt, 1e-5, ga_, ia, gb_, ib, x_ if fold else res_, round_hidden=True)

    (y64, yr64), gr = N.node(fn, (x, N.gemm_w(ps["w1"]), ps["b1"], N.gemm_w(ps["w2"]), ps["b2"], ps.get("gamma"), ps.get("beta"), ga, gb, other),
                             (dy[:, :O], dyr if res is not None else None))
    T = Tally(f"row_mlp {size} {config} (R = {R})")
    T.bar(rel(y[:, :O], y64), COMPOSED_BARS["row_mlp y"], "y", "row_mlp y", cap=UNIT_OUT)
    T.rows(y[:, :O], y64, "y", "row_mlp rows", ROW_BARS["row_mlp rows"])
    assert not y[:, O:].any()
    if yr is not None:
        base = (x if fold else other).detach().double()
        T.bar(rel(yr.double() - base, yr64 - base), COMPOSED_BARS["row_mlp y"], "y + res", "row_mlp y", cap=UNIT_OUT)
        T.rows(yr.double() - base, yr64 - base, "y + res", "row_mlp rows", ROW_BARS["row_mlp rows"])
    base = dyr.double() if fold else 0
    T.bar(rel(gi["x"].double() - base, gr[0] - base), COMPOSED_BARS["row_mlp dx"], "dx", "row_mlp dx", cap=UNIT_GRAD)
    T.rows(gi["x"].double() - base, gr[0] - base, "dx", "row_mlp grad rows", ROW_BARS["row_mlp grad rows"], own=False)
    for k, ref in (("w1", gr[1]), ("w2", gr[3])):
        T.bar(rel(pg[k], ref), COMPOSED_BARS["row_mlp dW"], f"d{k}", "row_mlp dW", cap=UNIT_GRAD)
    for k, ref in (("b1", gr[2]), ("b2", gr[4]), ("gamma", gr[5]), ("beta", gr[6])):
        if ref is not None:
            T.bar(rel(pg[k], ref), COMPOSED_BARS["row_mlp db"], f"d{k}", "row_mlp db", cap=UNIT_GRAD)
    for k, ref in (("ga", gr[7]), ("gb", gr[8])):
        if ref is not None:
            T.bar(rel(gi[k], ref), COMPOSED_BARS["row_mlp daddend"], f"d{k}", "row_mlp daddend", cap=UNIT_GRAD)
            T.rows(gi[k], ref, f"d{k}", "row_mlp grad rows", ROW_BARS["row_mlp grad rows"], own=False)
    if other is not None:
        same(gi["res"], dyr, "dres")
    T.done()


def _segment_case(dev, cus, dtype, split):
    """N just past the cap of the wanted split with an odd tail, E from the mean list length that selects it"""
    chunks = 64 * (2 if dtype == torch.bfloat16 else 4) // 16
    groups = 64 >> min(N._ceil_log2(chunks), 6)
    if split == "none":
        spw, mean = groups, 3
    else:
        spw, mean = 1, 40
    n = 4 * 16 * cus * spw + 3
    return n, mean * n + 11, chunks


@pytest.mark.parametrize("split", ["none", "largest"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_segment_sum_past_the_cap(gpu_device, dtype, split):
    """N past 16 x CUs workgroups: a wave takes a second batch of segments; without a split (mean list <= 4) and with the largest one (mean
    > 32); every 7th receiver and the last one empty, one receiver holding 5 % of all edges; the pair launch against its two launches"""
    from py4cast_amd.ops_graph import _segment_sum_pair_raw, _segment_sum_raw, aggregate_sum

    dev, cus = gpu_device, cus_of(gpu_device)
    n, E, chunks = _segment_case(dev, cus, dtype, split)
    blocks, lpr_log2, split_log2 = N.segment_sum_shape(n, E, chunks, cus)
    waves = N._cdiv(n, (64 >> lpr_log2) >> split_log2)
    assert N._cdiv(waves, 4) > 16 * cus == blocks and n % 32
    assert split_log2 == (0 if split == "none" else 6 - lpr_log2) and (N._cdiv(E, n) <= 4 if split == "none" else N._cdiv(E, n) > 32)
    gen = torch.Generator(device=dev).manual_seed(71)
    e = _edges(E, n // 2 + 5, n, dev, gen, hub=0.05, empty=True)
    deg = N.in_degree(e.dst, n)
    assert int((deg == 0).sum()) >= n // 8 and deg[n - 1] == 0 and int(deg.max()) >= 0.05 * E
    msg = torch.randn(E, 64, device=dev, generator=gen).to(dtype).requires_grad_(True)
    out = aggregate_sum(msg, e)
    dy = torch.randn(n, 64, device=dev, generator=gen).to(dtype)
    out.backward(dy)
    torch.cuda.synchronize()
    ref = N.segment_sum(msg.detach().double(), e.dst, n)
    T = Tally(f"segment_sum {dtype} split {split_log2} (N = {n}, E = {E})")
    d = out.detach().double() - ref
    if dtype == torch.bfloat16:
        T.bar(float(d.abs().max() / ref.abs().max()), 6e-3, "sum (max)", "bf16 map, max")
        T.bar(rel(out, ref), 3e-3, "sum (2-norm)", "bf16 map, 2-norm")
        T.rows(out[deg > 0], ref[deg > 0], "sum", "single-kernel rows", ROW_BARS["single-kernel rows"])
    else:
        T.bar(rel(out, ref), 1e-5, "sum", "fp32 out")
        T.rows(out[deg > 0], ref[deg > 0], "sum", "fp32 rows", ROW_BARS["fp32 rows"])
    assert not out[deg == 0].any(), "a receiver without edges is not zero"
    same(msg.grad, N.rows_of(dy, e.dst), "the adjoint gather")
    same(aggregate_sum(msg.detach(), e), out.detach(), "segment_sum, twice")
    a, b = _segment_sum_pair_raw(msg.detach(), e.by_src, e.n_src, e.by_dst, e.n_dst)
    same(a, _segment_sum_raw(msg.detach(), *e.by_src, e.n_src), "segment_sum_pair: the sender side against its own launch")
    same(b, out.detach(), "segment_sum_pair: the receiver side against its own launch")
    T.rows(a, N.segment_sum(msg.detach().double(), e.src, e.n_src), "pair, sender side", "single-kernel rows" if dtype == torch.bfloat16 else "fp32 rows",
           ROW_BARS["single-kernel rows" if dtype == torch.bfloat16 else "fp32 rows"])
    T.done()


@pytest.mark.parametrize("act", ["none", "relu", "silu"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_edge_gather_add_past_the_cap(gpu_device, dtype, act):
    """E past 16 x CUs workgroups x 4 waves x 2 row batches: a wave takes a second pair of batches; forward, and backward through the
    activation's derivative and the two segment sums"""
    from py4cast_amd.ops_graph import edge_gather_add

    dev, cus = gpu_device, cus_of(gpu_device)
    chunks = 8 if dtype == torch.bfloat16 else 16
    rpw = 64 >> N._ceil_log2(chunks)
    E = 2 * rpw * 4 * 16 * cus + 37
    assert N.gather_add_launch(E, cus, chunks).capped and not N.gather_add_launch(E - 37, cus, chunks).capped
    gen = torch.Generator(device=dev).manual_seed(81)
    ns, nr = E // 5 + 3, E // 11 + 1
    e = _edges(E, ns, nr, dev, gen)
    mk = lambda r: torch.randn(r, 64, device=dev, generator=gen).to(dtype).requires_grad_(True)  # noqa: E731
    base, a, b = mk(E), mk(ns), mk(nr)
    dy = torch.randn(E, 64, device=dev, generator=gen).to(dtype)
    y = edge_gather_add(base, a, b, e, act)
    y.backward(dy)
    torch.cuda.synchronize()
    y64, gr = N.node(lambda b_, a_, c_: N.edge_gather_add(b_, a_, e.src, c_, e.dst, act), (base, a, b), dy)
    T = Tally(f"edge_gather_add {dtype} {act} (E = {E})")
    bf = dtype == torch.bfloat16
    for got, ref, what, grad in ((y, y64, "y", False), (base.grad, gr[0], "dbase", True), (a.grad, gr[1], "da", True), (b.grad, gr[2], "db", True)):
        if bf:
            T.bar(float((got.detach().double() - ref).abs().max() / ref.abs().max()), 6e-3, f"{what} (max)", "bf16 map, max")
            T.bar(rel(got, ref), 3e-3, f"{what} (2-norm)", "bf16 map, 2-norm")
        else:
            T.bar(rel(got, ref), 1e-4 if grad else 1e-5, what, "fp32 grad" if grad else "fp32 out")
        if act != "relu" or what != "y":           # (ReLU zeroes whole stretches of a row, never a whole row of 64: every row has norm)
            T.rows(got, ref, what, "single-kernel rows" if bf else "fp32 rows", ROW_BARS["single-kernel rows" if bf else "fp32 rows"], own=not grad)
    same(edge_gather_add(base.detach(), a.detach(), b.detach(), e, act), y.detach(), "edge_gather_add, twice")
    T.done()


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("size", ["proj-cap", "wgrad-cap"])
def test_node_proj_past_the_caps(gpu_device, size, n):
    """R = 128 x 2 x CUs + 17 (forward / data gradient loop) and R = 512 x CUs + 33 (the weight gradient's waves take a fifth tile)"""
    from py4cast_amd.ops_nodeproj import node_proj

    dev, cus = gpu_device, cus_of(gpu_device)
    R = 128 * N.PROJ_PER_CU * cus + 17 if size == "proj-cap" else 512 * cus + 33
    f, _, w = N.proj_launches(R, cus)
    assert f.capped and w.capped == (size == "wgrad-cap") and R % 32
    gen = torch.Generator(device=dev).manual_seed(91)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    wide, aggr = (rn(64, 192) * 0.125).requires_grad_(True), (rn(64, 128) * 0.125).requires_grad_(True)
    x = _bf(rn(R, 64)).requires_grad_(True)
    dys = [_bf(rn(R, 64)) for _ in range(n)] + [_bf(rn(R, 64))]

    def once():
        wide.grad, aggr.grad, x.grad = torch.full_like(wide, 0.25), torch.full_like(aggr, -0.5), None
        outs = node_proj(x, [wide[:, 64:128], wide[:, 128:], aggr[:, :64]][:n], True, passthrough=True)
        assert type(outs[0].grad_fn).__name__ == "_NodeProjBackward"
        backward(outs, dys)
        return [o.detach() for o in outs], x.grad.clone(), wide.grad - 0.25, aggr.grad + 0.5

    outs, dx, gw, ga = once()
    outs2, dx2, gw2, ga2 = once()
    for i in range(n):
        same(outs2[i], outs[i], f"y{i}, twice")
    same(dx2, dx, "dx, twice"), same(gw2, gw, "dW (wide), twice"), same(ga2, ga, "dW (aggr), twice")
    ws = [N.gemm_w(t) for t in (wide[:, 64:128], wide[:, 128:], aggr[:, :64])][:n]
    ys, gr = N.node(lambda x_, *w_: N.node_proj(x_, w_, True), (x, *ws), dys)
    T = Tally(f"node_proj {size} n = {n} (R = {R})")
    for i in range(n):
        T.bar(float((outs[i].double() - ys[i]).abs().max() / ys[i].abs().max()), 6e-3, f"y{i} (max)", "bf16 map, max")
        T.bar(rel(outs[i], ys[i]), 3e-3, f"y{i} (2-norm)", "bf16 map, 2-norm")
        T.rows(outs[i], ys[i], f"y{i}", "node_proj rows", ROW_BARS["node_proj rows"])
        T.bar(rel([gw[:, 64:128], gw[:, 128:], ga[:, :64]][i], gr[1 + i]), 5e-4, f"dW{i}", "GEMM dW")
    same(outs[n], x.detach(), "the passthrough tensor")
    T.bar(float((dx.double() - gr[0]).abs().max() / gr[0].abs().max()), 6e-3, "dx (max)", "bf16 map, max")
    T.bar(rel(dx, gr[0]), 3e-3, "dx (2-norm)", "bf16 map, 2-norm")
    T.rows(dx, gr[0], "dx", "node_proj grad rows", ROW_BARS["node_proj grad rows"], own=False)
    untouched = [gw[:, :64]] + [t for i, t in enumerate((gw[:, 64:128], gw[:, 128:], ga[:, :64])) if i >= n] + [ga[:, 64:]]
    assert all(not t.any() for t in untouched), "a weight-gradient block that was not asked for changed"
    T.done()
