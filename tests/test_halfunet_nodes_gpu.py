"""
The HalfUNet plan (csrc/halfunet.cpp) node by node against float64: one forward + backward per case through the model, every buffer of
the plan's two workspaces read back at the offsets p4c_halfunet_layout reports (tests/halfunet_nodes.py::run_plan), and every node
checked ALONE from the stored buffers upstream of it -- per block, with the block, the quantity and the case in the message.

Forward: Y[i] (conv3x3 of the block's stored input), norm[i] (scale | shift | mean | rstd from the statistics of stored Y[i]; BatchNorm
rows equal for every sample; running statistics by torch's rule; eval mode from the running statistics), P[k] (max-pool), S (bilinear
up-sample-and-sum of the five levels), y (1x1 convolution).  Backward: the gradient buffer of every block holds either dA (gradient of
the ReLU output: pass 2 of the normalisation backward is fused into the consumers' loaders) or dY (written over dA in place) -- the
reader states which (halfunet_nodes.holds_dA) and both are checked; dgamma / dbeta / k1 / k2 / dW of every block, dW_out, dS, the x
passes tx_1..tx_4 of the up-sampling adjoints, dx (zero beyond grad_input_channels).  The rotating dP buffers do not survive the
call, so each encoder level is ONE composite node: dA of its second block = y pass of the adjoint of stored tx_k + max-pool routing
of dgrad(dY of the next level's first block) by the arg-max of the stored activations.  Every decision of a backward reference
comes from the device's stored values, so nothing is excluded from any comparison.  Wiring: every p.grad is its node's gradient,
37 parameters, each in exactly one node; the gradient-buffer set the call did not use still holds the sentinel in every byte.

Bars (tests/test_unet_nodes_gpu.py): bf16 maps <= 6e-3 of the largest magnitude per element and <= 3e-3 in the 2-norm, convolution
weight gradients <= 5e-4, gamma / beta gradients <= 5e-3, running mean / var <= 1e-4, fp32-stored nodes <= 1e-5 on outputs and
<= 1e-4 on gradients.  The bars without precedent (norm arrays, k1 / k2, tx_k, the composite level node) are 4 x the worst value
measured over all cases on one MI355X, rounded up to one digit, and never looser than the bf16-map bars (bf16 storage) or 1e-4
(fp32); they are set per storage type, since the two differ by four orders of magnitude.

Measured on one MI355X, worst over the cases / bar (the node it was met at):
  bf16 storage (small-64, rows-96, group-odd, eval, many-samples, wide-input)
    forward maps        5.0e-3 / 6e-3 per element, 2.3e-3 / 3e-3 2-norm   (Y[0] of rows-96 / small-64: the split first convolution
                                                                            stores the map twice -- two bf16 roundings; others 1.7e-3)
    gradient maps       4.0e-3 / 6e-3, 1.7e-3 / 3e-3                      (dY[4] of group-odd, dY[6] of small-64)
    dW                  3.3e-5 / 5e-4      dgamma 1.8e-4 / 5e-3      dbeta 1.6e-4 / 5e-3      running mean / var 4.9e-8 / 1e-4
    norm arrays         7.6e-8 / 4e-7                                     (norm[2].shift of many-samples)
    k1 / k2             1.8e-4 / 8e-4                                     (k2[6] of wide-input)
    tx_k                3.6e-3 / 6e-3, 1.7e-3 / 3e-3                      (one bf16 rounding of the stored map; 4 x exceeds the map bars)
    composite level     3.6e-3 / 6e-3, 1.8e-3 / 3e-3                      (dY[3] of wide-input, dY[9] of group-odd; likewise)
  fp32 storage (f32-store, f32)
    forward maps        4.5e-7 / 1e-5      gradient maps 4.3e-7 / 1e-4      dW 4.1e-7, dgamma 8.8e-7, dbeta 1.2e-6 / 1e-4
    running mean / var  1.5e-7 / 1e-4      norm arrays 2.2e-7 / 9e-7        k1 / k2 1.3e-6 / 6e-6
    tx_k                6.6e-8 / 3e-7      composite level 4.2e-7 / 2e-6
The whole file takes about 6 s on one MI355X.

Where a gradient buffer ends up holding dY, the dA the normalisation backward read is gone.  The reference then takes the dA it
derives from the stored buffers upstream and rounds it to the storage type, as the producer did when it stored it (the fused pass 1
of enc_out_bwd and of the data-gradient drains sums the packed values as well); likewise the dP that enc_out_bwd routes.  With the
unrounded float64 dA instead, the sums over a coarse map of a few hundred pixels carry the rounding noise of every element: k1 / k2
then measured up to 7.9e-3 and dbeta 7.3e-3 (blocks 1, 3, 5 of small-64, many-samples and wide-input).
"""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import halfunet_nodes as N  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (B, H, W, cin, cout, compute, storage, norm, grad_input_channels or None)
CASES = {
    "small-64": (2, 64, 64, 69, 60, "bf16", "bf16", "batch", None),
    "rows-96": (2, 256, 96, 69, 60, "bf16", "bf16", "batch", None),
    "group-odd": (3, 48, 80, 46, 21, "bf16", "bf16", "group", None),
    "eval": (2, 64, 64, 69, 60, "bf16", "bf16", "batch", None),          # small-64's model after its training call, .eval()
    "many-samples": (33, 16, 48, 69, 60, "bf16", "bf16", "batch", None),
    "wide-input": (2, 32, 64, 138, 60, "bf16", "bf16", "batch", 120),
    "f32-store": (2, 32, 64, 46, 21, "bf16", "f32", "batch", None),
    "f32": (2, 32, 48, 10, 1, "f32", "f32", "batch", None),
}

# quantity -> bar; "map" bars are (per element of the largest magnitude, 2-norm), every other one is the relative 2-norm
BARS_BF16 = {"map": (6e-3, 3e-3), "dW": 5e-4, "dgamma": 5e-3, "dbeta": 5e-3, "running": 1e-4,
             "norm": 4e-7, "k": 8e-4, "tx": (6e-3, 3e-3), "level": (6e-3, 3e-3)}
BARS_F32 = {"out": 1e-5, "grad": 1e-4, "dW": 1e-4, "dgamma": 1e-4, "dbeta": 1e-4, "running": 1e-4,
            "norm": 9e-7, "k": 6e-6, "tx": 3e-7, "level": 2e-6}


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def relmax(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def make_model(case, dev):
    from py4cast_amd.halfunet import HalfUNetMI355X, HalfUNetSettings

    B, H, W, cin, cout, compute, storage, norm, gic = CASES[case]
    torch.manual_seed(0)
    m = HalfUNetMI355X(cin, cout, (H, W), HalfUNetSettings(compute_dtype=compute, activation_dtype=storage, norm=norm, groups=8)).to(dev).train()
    if gic is not None:
        m.grad_input_channels = gic
    with torch.no_grad():   # non-trivial affine parameters, as tests/test_model_gpu.py::_make_pair
        for nb in m._norms:
            nb.weight.uniform_(0.5, 1.5)
            nb.bias.uniform_(-0.3, 0.3)
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(B, H, W, cin, device=dev, generator=g)
    gy = torch.randn(B, H, W, cout, device=dev, generator=g)   # unit scale
    return m, x, gy


def assert_route(case, m, B, H, W):
    """the route the case claims to reach, by the library's own predicates (skips where the CU count of the machine rules it out)"""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops_model as om

    lev = [(H >> k, W >> k) for k in range(5)]
    kind = [om.conv_kernel_kind(B, h, w) for h, w in lev]
    held = N.holds_dA(m, B, H, W)
    if case in ("small-64", "eval"):
        for h, w in lev:
            if not om.conv_small_ok(B, h, w):
                pytest.skip(f"{case}: the small kernel does not take {B} x {h} x {w} on this machine (CU count)")
        slots = [B * L.lib().p4c_conv_small_stat_slots(B, h, w) for h, w in lev[1:]]
        assert max(slots) <= 256, f"{case}: no statistics hand-off ({slots} slots)"
        assert W % 64 == 0 and m.cin_pad == 96 and kind[0] == 2
        assert held == [False, True] + [False] * 8 + [True, True], held
    elif case == "rows-96":
        assert B * H * W > 2 * 128 * 160 and not om.conv_small_ok(B, H, W) and kind[0] == 2, f"{case}: level 0 is not on the row kernel"
        assert W % 32 == 0 and 64 < m.in_channels <= 72 and m.cin_pad == 96          # first convolution split + thin weight-gradient chunk
        if not om.conv_small_ok(B, *lev[1]):
            pytest.skip(f"{case}: the small kernel does not take level 1 on this machine (CU count)")
        assert kind[1] == 2 and kind[2:] == [1, 1, 1], kind                          # level 1 row backward; W = 24, 12, 6 on the tile ring
        assert W % 64 != 0                                                           # generic up_bwd_x4
        assert held == [False, True, True, True] + [False] * 6 + [True, True], held
    elif case == "group-odd":
        assert m._settings.norm == "group" and B % 2 == 1 and lev[4] == (3, 5)
    elif case == "many-samples":
        assert B > 32 and not any(held), held                                        # norm_bwd_apply on every block
    elif case == "wide-input":
        assert m.cin_pad == 160 and m.dx_width == 128 and not held[0]
    elif case == "f32-store":
        assert m.act_dtype == torch.float32 and m.compute_dtype == torch.bfloat16 and not any(held)
    elif case == "f32":
        assert m.compute_dtype == torch.float32 and m.cin_pad == 32 and not any(held)
        assert L.lib().p4c_conv_kernel_kind(L.F32, L.F32, 64, 3, B, H, W) == 0


class Run(SimpleNamespace):
    def __repr__(self):   # (a failure report prints the fixture: not every tensor of the plan)
        return f"Run({self.case})"


@pytest.fixture(scope="module", params=list(CASES))
def run(request, gpu_device):
    case = request.param
    B, H, W, cin, cout, compute, storage, norm, _ = CASES[case]
    m, x, gy = make_model(case, gpu_device)
    assert_route(case, m, B, H, W)
    if case == "eval":
        N.run_plan(m, x, gy)        # the training call that leaves the running statistics
        m.eval()
    r = N.run_plan(m, x, gy)
    spec = N.Spec(bf16=compute == "bf16", norm=norm, groups=8, eps=1e-5, momentum=0.1, training=m.training)
    w, gamma, beta, wout = N.split_params([p.detach().clone() for p in m._ordered_params()])
    figures = []
    _forward(r, spec, w, gamma, beta, wout, cout, figures)
    _backward(r, spec, w, gamma, beta, wout, cout, m, figures)
    yield Run(case=case, r=r, spec=spec, figures=figures, bf16_store=storage == "bf16", model=m)
    del m, r, figures
    torch.cuda.empty_cache()


def _forward(r, spec, w, gamma, beta, wout, cout, fig):
    B = r.x.shape[0]
    A = lambda i: N.act(r.Y[i], r.norm[i][0], r.norm[i][1], as_device=True)   # noqa: E731
    r.inp = []
    for i in range(N.NCONV):
        if i == 0:
            inp = r.x[..., : w[0].shape[1]]
        elif i == 10:
            inp = r.S
        elif i % 2 == 0:
            inp = r.P[i // 2]
        else:
            inp = A(i - 1)
        r.inp.append(spec.q(inp))
        fig.append(("out", f"Y[{i}]", r.Y[i], N.conv(r.inp[i], spec.q(w[i]))))
        sc, sh, mean, rstd = r.norm[i]
        if spec.batch_stats:
            m64, v64, vu64 = N.norm_stats(r.Y[i], spec)
        else:
            m64, v64 = (N._per_sample(r.running_pre[i][j].double(), B) for j in (0, 1))
        for name, got, ref in zip(("scale", "shift", "mean", "rstd"), r.norm[i], N.norm_arrays(m64, v64, gamma[i], beta[i], spec.eps)):
            fig.append(("norm", f"norm[{i}].{name}", got, ref))
        if spec.norm == "batch":
            for name, a in zip(("scale", "shift", "mean", "rstd"), r.norm[i]):
                fig.append(("equal", f"norm[{i}].{name} rows of every sample", a, a[0:1].expand_as(a)))
        if spec.norm == "batch" and spec.training:
            rm, rv = N.running_update(r.running_pre[i][0], r.running_pre[i][1], m64, vu64, spec.momentum)
            fig.append(("running", f"running_mean[{i}]", r.running_post[i][0], rm))
            fig.append(("running", f"running_var[{i}]", r.running_post[i][1], rv))
        else:
            fig.append(("equal", f"running statistics [{i}] untouched", r.running_post[i], r.running_pre[i]))
    for k in range(1, N.NLEV):
        fig.append(("out", f"P[{k}]", r.P[k], N.pool(A(2 * k - 1))))
    fig.append(("out", "S", r.S, sum(N.upsample(A(2 * k + 1), 1 << k) for k in range(N.NLEV))))
    fig.append(("out", "y", r.y, N.conv(spec.q(A(11)), spec.q(wout))))


def _backward(r, spec, w, gamma, beta, wout, cout, model, fig):
    dy = spec.q(r.dy)   # (fp32 storage with bf16 matrix cores: the kernels round dy as they load it)
    A = lambda i: N.act(r.Y[i], r.norm[i][0], r.norm[i][1], as_device=True)   # noqa: E731
    grads = r.grads
    dYop = [None] * N.NCONV     # dY of block i as the matrix cores read it
    # a gradient map as its producer stored it: rounded to the storage type.  The normalisation backward of a block whose buffer ends
    # up holding dY read the STORED dA before it wrote dY over it (the fused pass 1 of enc_out_bwd and of the data-gradient drains sums
    # the packed values too), and enc_out_bwd reads the stored dP: the reference rounds where the device stored
    stored = lambda t: t.float().to(r.D[0].dtype).double()   # noqa: E731

    def block(i, dA_ref, kind):
        """the node of block i given the reference dA from the stored buffers upstream: the buffer's own check, then dgamma / dbeta /
        k1 / k2 / dW from the stored operands"""
        sc, sh, mean, rstd = r.norm[i]
        mask = N.preact(r.Y[i], sc, sh, as_device=True) > 0
        if r.holds_dA[i]:
            fig.append((kind, f"dA[{i}] (DY[{r.set}][{i}] holds dA)", r.D[i], dA_ref))
            g_in = r.D[i]
        else:
            g_in = stored(dA_ref)
        dgamma, dbeta, k1, k2, dY = N.norm_bwd(g_in, r.Y[i], mask, mean, rstd, gamma[i], spec)
        if not r.holds_dA[i]:
            fig.append((kind, f"dY[{i}] (DY[{r.set}][{i}] holds dY, in place)", r.D[i], dY))
        dYop[i] = spec.q(dY if r.holds_dA[i] else r.D[i])
        fig.append(("dgamma", f"dgamma[{i}]", grads[3 * i + 1], dgamma))
        fig.append(("dbeta", f"dbeta[{i}]", grads[3 * i + 2], dbeta))
        if spec.batch_stats:
            fig.append(("k", f"k1[{i}]", r.k1[i], k1))
            fig.append(("k", f"k2[{i}]", r.k2[i], k2))
        else:
            fig.append(("zero", f"k1[{i}] (eval: zero)", r.k1[i], torch.zeros_like(r.k1[i])))
            fig.append(("zero", f"k2[{i}] (eval: zero)", r.k2[i], torch.zeros_like(r.k2[i])))
        fig.append(("dW", f"dW[{i}]", grads[3 * i], N.conv_dw(r.inp[i], dYop[i])))
        return N.conv_dx(dYop[i], spec.q(w[i]))

    fig.append(("dW", "dW_out", grads[36], N.conv_dw(spec.q(A(11)), dy, 1)[:cout]))
    wo = torch.zeros(N.NF, N.NF, 1, 1, dtype=torch.float64, device=dy.device)
    wo[:cout] = spec.q(wout)
    dS = block(10, block(11, N.conv_dx(dy, wo), "grad"), "grad")
    fig.append(("grad", "dS (G0)", r.G0, dS))
    for k in range(1, N.NLEV):
        fig.append(("tx", f"tx_{k}", r.TX[k], N.up_adj_x(r.G0, 1 << k)))
    dP = None
    for k in range(N.NLEV - 1, -1, -1):
        dA = N.up_adj_y(r.TX[k] if k else r.G0, 1 << k)
        if dP is not None:
            dA = dA + N.pool_route(A(2 * k + 1), stored(dP))
        dP = block(2 * k, block(2 * k + 1, dA, "level"), "grad")
    dxc = model.dx_channels
    fig.append(("grad", "dx[..., :grad_input_channels]", r.dx[..., :dxc], dP[..., :dxc]))
    fig.append(("zero", "dx beyond grad_input_channels (zero)", r.dx[..., dxc:], torch.zeros_like(r.dx[..., dxc:])))
    assert len(grads) == 37 == len(list(model.parameters())), "every parameter belongs to exactly one node"


def _check(run, kinds):
    """asserts the figures of the given kinds against their bars; prints worst value / bar per kind"""
    bars = BARS_BF16 if run.bf16_store else BARS_F32
    worst, failures = {}, []
    for kind, what, got, ref in run.figures:
        if kind not in kinds:
            continue
        assert got.shape == ref.shape, f"{run.case}: {what}: shape {tuple(got.shape)} against {tuple(ref.shape)}"
        assert bool(torch.isfinite(got.float()).all()), f"{run.case}: {what}: not finite"
        if kind in ("equal", "zero"):
            if not torch.equal(got.double(), ref.double()):
                failures.append(f"{run.case}: {what}: not equal (max difference {float((got.double() - ref.double()).abs().max()):.3e})")
            continue
        key = kind
        if run.bf16_store and kind in ("out", "grad"):
            key = "map"
        bar = bars[key]
        if isinstance(bar, tuple):
            vals = ((relmax(got, ref), bar[0], "per element"), (rel(got, ref), bar[1], "2-norm"))
        else:
            vals = ((rel(got, ref), bar, "2-norm"),)
        for v, lim, how in vals:
            wk = f"{kind} ({how})"
            if v >= worst.get(wk, (-1.0,))[0]:
                worst[wk] = (v, lim, what)
            if not v <= lim:
                failures.append(f"{run.case}: {what}: {v:.3e} > {lim:.0e} ({how})")
    print(f"\n{run.case}: worst value / bar: " + ", ".join(f"{k} {v:.1e} / {lim:.0e} [{what}]" for k, (v, lim, what) in sorted(worst.items())))
    assert not failures, "\n".join(failures)


def test_forward_nodes(run):
    """Y[i], P[k], S and y from the stored buffers upstream of each, against the references' own decisions"""
    _check(run, {"out"})


def test_norm_arrays_and_running_statistics(run):
    _check(run, {"norm", "running", "equal"})


def test_backward_maps(run):
    """the gradient buffer of every block (dA or dY, whichever it holds), dS, tx_1..tx_4, the composite level nodes, dx"""
    _check(run, {"grad", "tx", "level", "zero"})


def test_parameter_gradients_and_coefficients(run):
    """p.grad of each of the 37 parameters is its own node's gradient; k1 / k2 of every block"""
    _check(run, {"dW", "dgamma", "dbeta", "k"})
