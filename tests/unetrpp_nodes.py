"""
Node-level oracle of the native UNETR++ transformer block (py4cast_amd/unetrpp.py): float64 references of the efficient paired attention
core (``ops_ts.epa_core``), the published x_SA merge (``ops_ts.merge_published``), the two output projections with the block's residual
and layer scale (``ops_gemm.cat_linear_res``), x + pos_embed with its LayerNorm (``ops_rows.add_layer_norm``) and conv51's batch norms
with LeakyReLU, residual, passthrough gradient and channel-dropout table (``ops_gemm.batch_norm_act``) -- the helpers of
tests/test_unetrpp_nodes_gpu.py (every such node inside the network), tests/test_unetrpp_gpu.py (epa_core alone) and
tests/test_unetrpp_nodes_cpu.py (the references themselves, composed into the oracle's block).

References: float64 on the bf16 operands the device read, as tests/unet_nodes.py.  A weight is rounded to bf16 only where the kernel
reads a bf16 image of it: E's weight (the token-axis projection reads ``weight_as(W, bf16)``), out_proj / out_proj2 scaled by gamma
(``scaled_images``: the product gamma * W is rounded, so the reference rounds gamma * W, not W).  The biases, the temperatures and
gamma stay fp32 values, promoted.

Intermediates the device stores or reads in bf16 and the reference rounds there too (``rnd=True``; with ``rnd=False`` the reference is
the exact float64 algebra of oracle/unetrpp.py::EPA, which the CPU test proves):
* S = softmax(q Mq), the spatial branch's probabilities (the epilogue of p4c_ts_apply_softmax writes them in bf16; x_sa and the
  gradient of VP read that S);
* dL = S (dS - rowsum(S dS)), the spatial branch's softmax adjoint (written in bf16 by the same kernel's backward epilogue; dq's first
  contribution and the gradient of Mq read it), computed from the stored S;
* the small matrices the apply kernels multiply with on the matrix cores, which they stage as bf16 images: At (x_ca = v_ca At, and
  dv_ca = dx_ca A), Mq = t2 KP / nq (the logits q Mq, and dq = dL Mq^T), VP (x_sa = S VP^T, and dS = dx_sa VP).  Straight through: the
  gradients of these matrices are those of the unrounded ones (the kernels' gram products of them are fp32);
* g = (dKP, dVP), the token projection's gradient, where its adjoint applies read it (dk / dv_sa = W^T g^T and E.weight's gradient
  X g: bf16 images); E.bias's gradient sums the fp32 g.
Not modelled, and the reason the bars of dq and dk are wider (EPA_BARS below): the bf16 images of dG and 2 diag(dn) in their last two
applies, and the bf16 rounding of dq / dk between their accumulating applies.  G, the column norms, KP, VP, Mq, the softmax A and every
other gradient of the small matrices are fp32.

LayerNorm node: the table's gradient is summed from the bf16 dt the backward kernel stores (ops_rows._AddLayerNorm: dt is a bf16
tensor, p4c_sum_leading / the tensor-library sum read it); ``aln_node`` rounds dt there too (``rnd=True``).
"""
from collections import namedtuple

import torch

EPS = 1e-12     # F.normalize's clamp of the column norms

EPAREF = namedtuple("EPAREF", "x_sa x_ca dqkvv dW dbias dt1 dt2")


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _SoftmaxStored(torch.autograd.Function):
    """row softmax whose probabilities are rounded to bf16 as the device stores them, and whose backward takes those stored
    probabilities and rounds the logits' gradient to bf16 (the named roundings S and dL of the module docstring)"""

    @staticmethod
    def forward(ctx, z):
        s = _bf(z.softmax(dim=-1))
        ctx.save_for_backward(s)
        return s

    @staticmethod
    def backward(ctx, ds):
        (s,) = ctx.saved_tensors
        return _bf(s * (ds - (s * ds).sum(dim=-1, keepdim=True)))


def _image(t):
    """t as the bf16 image an apply kernel stages, with the gradient of t itself (straight through)"""
    return t + (_bf(t) - t).detach()


class _GradImage(torch.autograd.Function):
    """identity forward; backward: the bf16 image of the gradient (the projection's adjoint applies stage g = (dKP, dVP) as bf16)"""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return _bf(g)


def epa_forward(qkvv, W, bias, t1, t2, rnd=True):
    """(x_sa, x_ca), both (B, heads, N, d), of float64 qkvv (B, N, 4, heads, d), E = (W (p, N), bias (p,)), temperatures t1, t2
    (heads, 1, 1): oracle/unetrpp.py::EPA's algebra up to the projections, token-major per head"""
    q, k, vca, vsa = (qkvv[:, :, i].permute(0, 2, 1, 3) for i in range(4))          # (B, h, N, d)
    nq = q.norm(dim=2).clamp_min(EPS)                                                # (B, h, d): column norms over the tokens
    nk = k.norm(dim=2).clamp_min(EPS)
    qn, kn = q / nq.unsqueeze(2), k / nk.unsqueeze(2)
    img = _image if rnd else (lambda t: t)
    A = ((qn.transpose(-1, -2) @ kn) * t1).softmax(dim=-1)                           # (B, h, d, d) channel attention
    x_ca = vca @ img(A).transpose(-1, -2)                                            # (B, h, N, d)
    gimg = _GradImage.apply if rnd else (lambda t: t)
    KP = gimg(k.transpose(-1, -2) @ W.t()) + bias                                    # (B, h, d, p) = E(k)
    VP = gimg(vsa.transpose(-1, -2) @ W.t()) + bias                                  # = E(v_sa) (F = E)
    Mq = KP / nq.unsqueeze(-1) * t2                                                  # (B, h, d, p): q_hat KP t2 = q Mq
    z = q @ img(Mq)                                                                  # (B, h, N, p)
    S = _SoftmaxStored.apply(z) if rnd else z.softmax(dim=-1)
    x_sa = S @ img(VP).transpose(-1, -2)                                             # (B, h, N, d)
    return x_sa, x_ca


def epa_node(qkvv, W, bias, t1, t2, dx_sa=None, dx_ca=None, rnd=True, round_weight=True):
    """float64 EPA core node: EPAREF with the outputs and, given the incoming gradients, dqkvv / dW / dbias / dt1 / dt2 (else None).
    round_weight: E's weight rounded to bf16 first, as the token-axis projection reads it"""
    Wd = W.detach().to(torch.bfloat16) if round_weight else W.detach()
    ins = [t.detach().double().requires_grad_(True) for t in (qkvv, Wd, bias, t1, t2)]
    with torch.enable_grad():
        x_sa, x_ca = epa_forward(*ins, rnd=rnd)
    if dx_sa is None:
        return EPAREF(x_sa.detach(), x_ca.detach(), None, None, None, None, None)
    g = torch.autograd.grad((x_sa, x_ca), ins, (dx_sa.double(), dx_ca.double()))
    return EPAREF(x_sa.detach(), x_ca.detach(), *g)


def merge_published(x_sa):
    """the published code's x_SA merge: (B, h, N, d) -> ``permute(0, 3, 1, 2).reshape(B, N, C)`` (an exact permutation)"""
    B, H, N, d = x_sa.shape
    return x_sa.permute(0, 3, 1, 2).reshape(B, N, H * d)


def merge_restated(x_sa):
    """the restated block's merge: head-major per token"""
    B, H, N, d = x_sa.shape
    return x_sa.permute(0, 2, 1, 3).reshape(B, N, H * d)


CATLIN = namedtuple("CATLIN", "y dxa dwa dba dxb dwb dbb dres dgamma")


def catlin_node(xa, wa, ba, xb, wb, bb, res, gamma, dy=None, round_weight=True):
    """float64 res + gamma * cat(xa wa^T + ba, xb wb^T + bb): CATLIN (gradients None without dy).  round_weight: gamma * W rounded
    to bf16 (the kernel's scaled weight image), the bias term gamma * b in fp32 (scaled_images keeps it fp32)"""
    h = wa.shape[0]
    leaves = [t.detach().double().requires_grad_(True) for t in (xa, wa, ba, xb, wb, bb, res, gamma)]
    xa6, wa6, ba6, xb6, wb6, bb6, r6, g6 = leaves
    with torch.enable_grad():
        ga, gb = g6[:h], g6[h:]
        swa, swb = ga.unsqueeze(1) * wa6, gb.unsqueeze(1) * wb6
        if round_weight:       # the rounding of the image, with the gradient of the unrounded product (straight through)
            swa = swa + (_bf(swa) - swa).detach()
            swb = swb + (_bf(swb) - swb).detach()
        y = r6 + torch.cat([xa6 @ swa.t() + ga * ba6, xb6 @ swb.t() + gb * bb6], dim=-1)
    if dy is None:
        return CATLIN(y.detach(), *([None] * 8))
    return CATLIN(y.detach(), *torch.autograd.grad(y, leaves, dy.double()))


ALN = namedtuple("ALN", "t ln dx dadd dgamma dbeta")


def aln_node(x, add, gamma, beta, eps, t_stored=None, dt=None, dln=None, rnd=True):
    """float64 t = x + add, ln = LayerNorm(t): ALN.  add (the positional table, (1, N, C) or (N, C)) is read as its bf16 image.  The
    backward (dln given) runs on the STORED t (the kernel's operand; the module's own t without it) and adds dt (the residual's gradient,
    None for none); the table's gradient is the sum of dt_total over the leading dimension (of its bf16 rounding: rnd)"""
    C = x.shape[-1]
    N = add.numel() // C
    a64 = add.detach().to(torch.bfloat16).double().reshape(N, C)
    t = (x.detach().double().reshape(-1, N, C) + a64).reshape(x.shape)
    g64, b64 = gamma.detach().double(), beta.detach().double()
    ln = torch.nn.functional.layer_norm(t, (C,), g64, b64, eps)
    if dln is None:
        return ALN(t, ln, None, None, None, None)
    ts = (t if t_stored is None else t_stored.detach().double()).requires_grad_(True)
    gl, bl = g64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
    with torch.enable_grad():
        y = torch.nn.functional.layer_norm(ts, (C,), gl, bl, eps)
    dts, dg, db = torch.autograd.grad(y, (ts, gl, bl), dln.double())
    dx = dts if dt is None else dts + dt.double()
    dxs = _bf(dx) if rnd else dx
    return ALN(t, ln, dx, dxs.reshape(-1, N, C).sum(0).view(add.shape), dg, db)


def _max_rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def epa_measure(x_sa, x_ca, dqkvv, dW, dbias, dt1, dt2, ref: EPAREF):
    """{quantity: value} of an epa_core call against its reference: the bf16 maps (x_sa, x_ca, the four slices of dqkvv each against its
    own magnitude) per element against the largest magnitude ("max") and in the 2-norm, then E's and the temperatures' gradients"""
    out = {}
    maps = [("x_sa", x_sa, ref.x_sa), ("x_ca", x_ca, ref.x_ca)]
    maps += [(f"d{n}", dqkvv[:, :, i], ref.dqkvv[:, :, i]) for i, n in enumerate(("q", "k", "v_ca", "v_sa"))]
    for name, a, b in maps:
        out[f"{name} max"] = _max_rel(a, b)
        out[f"{name} 2-norm"] = _rel(a, b)
    out["dE.weight"], out["dE.bias"] = _rel(dW, ref.dW), _rel(dbias, ref.dbias)
    out["dtemperature"], out["dtemperature2"] = _rel(dt1, ref.dt1), _rel(dt2, ref.dt2)
    return out


# the bars of epa_measure's quantities: the suite's (bf16 maps 6e-3 per element / 3e-3 in the 2-norm, weight and bias gradients 5e-4,
# temperatures 5e-3), except dq and dk, whose last roundings are not modelled (module docstring): their bars were set from the first GPU
# runs, at most twice the worst value measured over the benchmark's EPA shapes and the node test's cases
EPA_BARS = {**{f"{n} max": 6e-3 for n in ("x_sa", "x_ca", "dv_ca", "dv_sa")},
            **{f"{n} 2-norm": 3e-3 for n in ("x_sa", "x_ca", "dv_ca", "dv_sa")},
            "dq max": 1.2e-2, "dk max": 1.2e-2, "dq 2-norm": 5e-3, "dk 2-norm": 5e-3,
            "dE.weight": 5e-4, "dE.bias": 5e-4, "dtemperature": 5e-3, "dtemperature2": 5e-3}


BNA = namedtuple("BNA", "out mean var var_unbiased dy dres dgamma dbeta")


def bn_act_node(y, gamma, beta, eps, slope, res=None, mul=None, factor=1.0, out_stored=None, dout=None, dpass=None):
    """float64 training-mode ``leaky_relu(BatchNorm2d(y) (+ res), slope) * mul[sample, channel] * factor`` of a features-last y
    (B, H, W, C): BNA.  mul (B, C) is the channel dropout's draw as the call was given it (None: no multiplier); factor 1 / (1 - p).
    The forward decides the LeakyReLU sign on its own values.  The backward (dout given) takes the sign from the device's stored output
    (out_stored > 0; where mul is 0 the gradient is 0 whatever the sign) and adds ``dpass`` -- the gradient the residual's passthrough
    output received from its later consumers -- to the residual's gradient, as the kernel does inside its backward launch."""
    B, C = y.shape[0], y.shape[-1]
    r = y.detach().double().reshape(B, -1, C)
    N = r.shape[0] * r.shape[1]
    flat = r.reshape(N, C)
    mean, var = flat.mean(0), flat.var(0, unbiased=False)
    rstd = torch.rsqrt(var + eps)
    g, bt = gamma.detach().double(), beta.detach().double()
    xhat = (r - mean) * rstd
    z = xhat * g + bt
    if res is not None:
        z = z + res.detach().double().reshape(B, -1, C)
    m = torch.ones(B, 1, C, dtype=torch.float64, device=y.device) if mul is None else mul.detach().double().view(B, 1, C) * factor
    out = (torch.where(z > 0, z, float(slope) * z) * m).view(y.shape)
    dy = dres = dgamma = dbeta = None
    if dout is not None:
        pos = (z > 0) if out_stored is None else (out_stored.detach().reshape(B, -1, C) > 0)
        dz = dout.detach().double().reshape(B, -1, C) * m * torch.where(pos, z.new_tensor(1.0), z.new_tensor(float(slope)))
        dbeta, dgamma = dz.sum((0, 1)), (dz * xhat).sum((0, 1))
        dy = (g * rstd * (dz - dbeta / N - xhat * (dgamma / N))).view(y.shape)
        if res is not None:
            dres = dz.view(y.shape) if dpass is None else dz.view(y.shape) + dpass.detach().double()
    vu = flat.var(0, unbiased=True)
    return BNA(out, mean, var, vu, dy, dres, dgamma, dbeta)
