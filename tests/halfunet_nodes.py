"""
Node-level oracle of the HalfUNet plan (csrc/halfunet.cpp: p4c_halfunet_forward / p4c_halfunet_backward): float64 references of every
step of the plan and a reader of the two workspaces -- the helpers of tests/test_halfunet_nodes_gpu.py (the device) and
tests/test_halfunet_nodes_cpu.py (the references themselves, against oracle.halfunet.HalfUNetRef under autograd).

The plan is one C call; its nodes are buffers at the offsets p4c_halfunet_layout reports.  Blocks 0..11: encoder level k convolution j
is 2k + j, the decoder's are 10 and 11; a block is conv3x3 -> norm -> ReLU and stores only the RAW convolution output Y[i] and the
normalisation arrays (scale | shift | mean | rstd, (B,64) each) -- the activation relu(Y * scale + shift) is formed by whoever reads
Y next.

References (the convention of tests/unet_nodes.py): float64 on the operands the device stored, features-last (B,H,W,C), on CPU or GPU
tensors alike.  Where a kernel rounds an operand to bf16 before the matrix core (weights, activations, the dY a fused loader forms in
fp32) the reference rounds the same operand (`Spec.q`).  For a backward every decision comes from the device's stored values: the ReLU
mask is stored Y * scale + shift > 0 evaluated as the kernels evaluate it (one fp32 fused multiply-add), the pool routing goes to the
first maximum in row-major order of the stored activations.  Forward outputs are checked against the references' own decisions.
A gradient map the device stored and later overwrote (dA where the buffer ends up holding dY, the rotating dP) is re-derived from the
stored buffers upstream and rounded to the storage type as its producer rounded it (tests/test_halfunet_nodes_gpu.py::_backward).
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

NCONV, NLEV, NF = 12, 5, 64
LEVEL = [i // 2 if i < 10 else 0 for i in range(NCONV)]


class Spec:
    """flavour of a plan: bf16 matrix cores or exact fp32; BatchNorm ("batch") or GroupNorm ("group"); training or eval statistics"""

    def __init__(self, bf16=False, norm="batch", groups=8, eps=1e-5, momentum=0.1, training=True):
        self.bf16, self.norm, self.groups, self.eps, self.momentum, self.training = bf16, norm, groups, eps, momentum, training

    @property
    def batch_stats(self):
        """the statistics of the call's own batch are in use (GroupNorm always; BatchNorm in training mode)"""
        return self.norm == "group" or self.training

    def q(self, t):
        """an operand as the matrix core reads it: rounded to bf16 (from the fp32 value the kernel holds), or exact"""
        t = t.detach().double()
        return t.float().bfloat16().double() if self.bf16 else t


# ------------------------------------------------------------------------------------------------ convolutions


def conv(x, w):
    """'same' 3x3 / 1x1 convolution of a float64 features-last x (B,H,W,Ci) with w (Co,Ci,k,k): one matmul per tap"""
    B, H, W, Ci = x.shape
    Co, k = w.shape[0], w.shape[2]
    if k == 1:
        return (x.reshape(-1, Ci) @ w.reshape(Co, Ci).t()).view(B, H, W, Co)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    y = 0
    for ky in range(3):
        for kx in range(3):
            y = y + (xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Ci) @ w[:, :, ky, kx].t()).view(B, H, W, Co)
    return y


def conv_dx(dy, w):
    """data gradient of conv: dx (B,H,W,Ci) = correlation of dy (B,H,W,Co) with the taps of w mirrored and its channels swapped"""
    return conv(dy, w.transpose(0, 1).flip(2, 3).contiguous())


def conv_dw(x, dy, k=3):
    """weight gradient of conv: (Co,Ci,k,k) from the convolution's input x (B,H,W,Ci) and the gradient dy (B,H,W,Co) of its output"""
    B, H, W, Ci = x.shape
    Co = dy.shape[-1]
    d = dy.reshape(-1, Co)
    if k == 1:
        return (d.t() @ x.reshape(-1, Ci)).view(Co, Ci, 1, 1)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    dw = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = d.t() @ xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Ci)
    return dw


# ------------------------------------------------------------------------------------------------ normalisation


def _per_sample(v, B):
    return v.unsqueeze(0).expand(B, -1).contiguous()


def norm_stats(Y, spec):
    """(mean, biased variance, unbiased variance or None) as (B,C) float64 arrays of a raw convolution output Y (B,H,W,C): BatchNorm
    over (B,H,W) per channel, the row repeated for every sample; GroupNorm over (H,W, channels of the group) per sample"""
    B, H, W, C = Y.shape
    y = Y.detach().double()
    if spec.norm == "batch":
        r = y.reshape(-1, C)
        n = r.shape[0]
        mean, var = r.mean(0), r.var(0, unbiased=False)
        return _per_sample(mean, B), _per_sample(var, B), _per_sample(var * n / (n - 1), B)
    cpg = C // spec.groups
    r = y.reshape(B, H * W, spec.groups, cpg).permute(0, 2, 1, 3).reshape(B, spec.groups, -1)
    mean, var = r.mean(-1), r.var(-1, unbiased=False)
    return mean.repeat_interleave(cpg, 1), var.repeat_interleave(cpg, 1), None


def norm_arrays(mean, var, gamma, beta, eps):
    """(scale, shift, mean, rstd) (B,C) of a normalisation with statistics mean / var (B,C): out = Y * scale + shift"""
    rstd = torch.rsqrt(var.double() + eps)
    scale = gamma.detach().double() * rstd
    return scale, beta.detach().double() - mean.double() * scale, mean.double(), rstd


def running_update(pre_mean, pre_var, mean, var_unbiased, momentum):
    """torch's BatchNorm2d rule for one training call: running <- (1 - m) running + m (batch mean / unbiased batch variance)"""
    return (1 - momentum) * pre_mean.double() + momentum * mean[0], (1 - momentum) * pre_var.double() + momentum * var_unbiased[0]


def _bc(v):
    return v.double()[:, None, None, :]


def preact(Y, scale, shift, as_device=False):
    """Y * scale + shift (float64).  as_device: the value a kernel holds -- the exact product and sum rounded once to fp32 (a fused
    multiply-add of fp32 operands: the float64 product of two fp32 numbers is exact)"""
    z = Y.detach().double() * _bc(scale) + _bc(shift)
    return z.float().double() if as_device else z


def act(Y, scale, shift, as_device=False):
    return torch.relu(preact(Y, scale, shift, as_device))


def norm_bwd(g_in, Y, mask, mean, rstd, gamma, spec):
    """float64 backward of [norm -> ReLU] for the gradient g_in of the activation: (dgamma, dbeta, k1, k2, dY) with
    dY = rstd (gamma g - k1 - xhat k2), g = g_in where mask, k1 / k2 (B,C) the mean over the statistics group of gamma g and of
    gamma g xhat -- zero when the statistics are constants (eval-mode BatchNorm: dY = scale g)"""
    B, H, W, C = Y.shape
    g = torch.where(mask, g_in.detach().double(), torch.zeros((), dtype=torch.float64, device=Y.device))
    xhat = (Y.detach().double() - _bc(mean)) * _bc(rstd)
    ga = gamma.detach().double()
    s1, s2 = g.sum((1, 2)), (g * xhat).sum((1, 2))   # (B,C)
    dbeta, dgamma = s1.sum(0), s2.sum(0)
    if not spec.batch_stats:
        k1 = k2 = torch.zeros(B, C, dtype=torch.float64, device=Y.device)
    elif spec.norm == "batch":
        n = B * H * W
        k1, k2 = _per_sample(ga * dbeta / n, B), _per_sample(ga * dgamma / n, B)
    else:
        cpg = C // spec.groups
        n = H * W * cpg
        k1 = ((ga * s1).view(B, spec.groups, cpg).sum(-1) / n).repeat_interleave(cpg, 1)
        k2 = ((ga * s2).view(B, spec.groups, cpg).sum(-1) / n).repeat_interleave(cpg, 1)
    dY = _bc(rstd) * (ga * g - _bc(k1) - xhat * _bc(k2))
    return dgamma, dbeta, k1, k2, dY


# ------------------------------------------------------------------------------------------------ pool and up-sampling


def _windows(t):
    """(B,H,W,C) -> (B,H/2,W/2,C,4): the 2x2 windows in row-major order (0,0) (0,1) (1,0) (1,1)"""
    B, H, W, C = t.shape
    return t.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)


def _unwindows(t):
    B, Ho, Wo, C, _ = t.shape
    return t.reshape(B, Ho, Wo, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * Ho, 2 * Wo, C)


def _first_max(win):
    """index of the first maximum along the last axis (an explicit scan: argmax's choice among equal values is not specified)"""
    best, arg = win[..., 0], torch.zeros(win.shape[:-1], dtype=torch.long, device=win.device)
    for q in range(1, win.shape[-1]):
        better = win[..., q] > best
        best = torch.where(better, win[..., q], best)
        arg = torch.where(better, torch.full_like(arg, q), arg)
    return arg


def pool(a):
    """2x2 / stride-2 max of a float64 activation map"""
    return _windows(a).amax(-1)


def pool_route(a_decide, dP):
    """adjoint of the 2x2 max-pool: dP (B,H/2,W/2,C) goes to the first maximum in row-major order of each window of a_decide"""
    arg = _first_max(_windows(a_decide))
    routed = torch.zeros(*arg.shape, 4, dtype=torch.float64, device=dP.device)
    routed.scatter_(-1, arg.unsqueeze(-1), dP.detach().double().unsqueeze(-1))
    return _unwindows(routed)


def pool_margin(a):
    """smallest gap between the largest and the second largest value of a 2x2 window (0: some window ties)"""
    top = _windows(a).topk(2, -1).values
    return float((top[..., 0] - top[..., 1]).min())


def up_matrix(n, s, device):
    """(n*s, n) float64 matrix of torch's bilinear up-sampling by s along one axis, align_corners=False:
    src = (dst + 0.5) / s - 0.5 clamped at 0, taps floor(src) and min(floor(src) + 1, n - 1)"""
    dst = torch.arange(n * s, dtype=torch.float64, device=device)
    src = ((dst + 0.5) / s - 0.5).clamp_min(0.0)
    i0 = src.floor().long().clamp_max(n - 1)
    i1 = (i0 + 1).clamp_max(n - 1)
    lam = src - i0
    U = torch.zeros(n * s, n, dtype=torch.float64, device=device)
    rows = torch.arange(n * s, device=device)
    U.index_put_((rows, i0), 1.0 - lam, accumulate=True)
    U.index_put_((rows, i1), lam, accumulate=True)
    return U


def upsample(a, s):
    """bilinear up-sampling by s of a (B,h,w,C) float64 map"""
    if s == 1:
        return a
    Uy, Ux = up_matrix(a.shape[1], s, a.device), up_matrix(a.shape[2], s, a.device)
    return torch.einsum("yY,xX,bYXc->byxc", Uy, Ux, a)


def up_adj_x(dS, s):
    """x pass of the adjoint of the up-sampling by s: (B,H,W,C) -> (B,H,W/s,C)"""
    return torch.einsum("xX,byxc->byXc", up_matrix(dS.shape[2] // s, s, dS.device), dS.detach().double())


def up_adj_y(tx, s):
    """y pass of that adjoint: (B,H,w,C) -> (B,H/s,w,C)"""
    if s == 1:
        return tx.detach().double()
    return torch.einsum("yY,byXc->bYXc", up_matrix(tx.shape[1] // s, s, tx.device), tx.detach().double())


# ------------------------------------------------------------------------------------------------ parameters


def split_params(params):
    """[w0, gamma0, beta0, ..., w11, gamma11, beta11, wout] (the plan's parameter order) -> (w, gamma, beta, wout)"""
    params = list(params)
    assert len(params) == 3 * NCONV + 1
    return params[0:36:3], params[1:36:3], params[2:36:3], params[36]


# ------------------------------------------------------------------------------------------------ the workspace reader

SENTINEL = 0xA5


def holds_dA(model, B, H, W):
    """Per block: True when its gradient buffer DY[set][i] holds dA (the gradient of the block's ReLU output) after the call, False
    when the normalisation backward wrote dY over it in place.  csrc/halfunet.cpp conv_block_bwd (`nbf`): pass 2 is left to the fused
    loaders of the data- and weight-gradient kernels -- and no dY map is written -- for a 64-channel input on bf16 maps the
    row-streaming kernel takes (W > 32, H >= 8) with B <= 32; the first convolution needs one 64-channel data-gradient block
    (dx_blocks = 1) and cin_pad = 64 besides.  (Read from the product library: the A/B switches of the diagnostic build change it.)"""
    from py4cast_amd import ops_model as om

    both_bf16 = model.compute_dtype == torch.bfloat16 and model.act_dtype == torch.bfloat16
    dx_blocks = max(1, (model.dx_channels + 63) // 64)
    out = []
    for i in range(NCONV):
        h, w = H >> LEVEL[i], W >> LEVEL[i]
        fused = both_bf16 and B <= 32 and om.conv_kernel_kind(B, h, w) == 2
        out.append(bool(fused and (i > 0 or (dx_blocks == 1 and model.cin_pad == NF))))
    return out


def _view(buf, off, dtype, shape):
    n = 1
    for s in shape:
        n *= s
    return buf[off: off + n * torch.empty((), dtype=dtype).element_size()].view(dtype).view(shape)


def run_plan(model, x, gy):
    """One forward and one backward of the plan through the model (as tests/test_small_conv_gpu.py::_plan_run fishes `saved` out of the
    autograd node), both gradient-buffer sets filled with a sentinel byte in between.  Returns the typed CLONES of every buffer of the
    layout, the set the backward used (the one that changed; the other must still hold the sentinel in every byte), what the kernels
    were handed (x padded, dy with zero columns beyond cout), the network's y, x.grad, every p.grad and the running statistics
    before / after."""
    from py4cast_amd import ops_model as om

    B, H, W, _ = x.shape
    dev = x.device
    desc = model._desc(B, H, W)
    lay = om.halfunet_layout(desc)
    act_dt = model.act_dtype
    esz = lay["elem_bytes"]
    assert esz == torch.empty((), dtype=act_dt).element_size()
    for p in model.parameters():
        p.grad = None
    running_pre = model._running_stats(dev).clone()
    xg = x.detach().clone().requires_grad_(True)
    y = model(xg)
    node, saved, x_seen = y.grad_fn, None, None
    while node is not None and saved is None:   # behind the channel slice and the cast to the caller's dtype: the plan's node
        st = getattr(node, "saved_tensors", ())
        if any(t.dtype == torch.uint8 for t in st):
            saved = next(t for t in st if t.dtype == torch.uint8)
            x_seen = next(t for t in st if t.dtype != torch.uint8)
        node = node.next_functions[0][0] if node.next_functions else None
    assert saved is not None and saved.numel() == lay["saved_bytes"], "the plan's saved workspace was not found behind y"
    _, scratch = model._workspaces(desc, dev)
    assert scratch.numel() == lay["scratch_bytes"]
    torch.cuda.synchronize()
    running_post = model._running.clone()
    n = [B * (H >> k) * (W >> k) * NF for k in range(NLEV)]
    shape = [(B, H >> k, W >> k, NF) for k in range(NLEV)]
    # both sets of gradient buffers and of k1 / k2: sentinel bytes
    regions = {s: [(lay["DY"][s][i], n[LEVEL[i]] * esz) for i in range(NCONV)] +
                  [(lay[k][s][i], B * NF * 4) for k in ("k1", "k2") for i in range(NCONV)] for s in (0, 1)}
    for s in (0, 1):
        for off, size in regions[s]:
            scratch[off: off + size] = SENTINEL
    dy_seen = torch.zeros(B, H, W, NF, dtype=act_dt, device=dev)
    dy_seen[..., : model.out_channels] = gy.to(y.dtype).to(act_dt)
    y.backward(gy.to(y.dtype))
    torch.cuda.synchronize()
    changed = [any(bool((scratch[off: off + size] != SENTINEL).any()) for off, size in regions[s]) for s in (0, 1)]
    assert changed[0] != changed[1], f"the backward wrote to gradient-buffer sets {changed}: exactly one was expected"
    used = 0 if changed[0] else 1
    for off, size in regions[1 - used]:
        assert bool((scratch[off: off + size] == SENTINEL).all()), f"the backward used set {used} and wrote into set {1 - used} at byte {off}"
    f32 = torch.float32
    r = SimpleNamespace(desc=desc, lay=lay, set=used, x=x_seen.detach().clone(), dy=dy_seen, y=y.detach().clone(), dx=xg.grad.clone(),
                        running_pre=running_pre.view(NCONV, 2, NF), running_post=running_post.view(NCONV, 2, NF),
                        grads=[p.grad.detach().clone() for p in model._ordered_params()], holds_dA=holds_dA(model, B, H, W))
    r.Y = [_view(saved, lay["Y"][i], act_dt, shape[LEVEL[i]]).clone() for i in range(NCONV)]
    r.P = [None] + [_view(saved, lay["P"][k], act_dt, shape[k]).clone() for k in range(1, NLEV)]
    r.S = _view(saved, lay["S"], act_dt, shape[0]).clone()
    r.norm = [tuple(_view(saved, lay["norm"][i] + j * B * NF * 4, f32, (B, NF)).clone() for j in range(4)) for i in range(NCONV)]
    r.G0 = _view(scratch, lay["G0"], act_dt, shape[0]).clone()
    r.TX, off = [None], lay["TB"]
    for k in range(1, NLEV):
        r.TX.append(_view(scratch, off, act_dt, (B, H, W >> k, NF)).clone())
        off += (n[0] >> k) * esz
    r.D = [_view(scratch, lay["DY"][used][i], act_dt, shape[LEVEL[i]]).clone() for i in range(NCONV)]
    r.k1 = [_view(scratch, lay["k1"][used][i], f32, (B, NF)).clone() for i in range(NCONV)]
    r.k2 = [_view(scratch, lay["k2"][used][i], f32, (B, NF)).clone() for i in range(NCONV)]
    return r


# ------------------------------------------------------------------------------------------------ the references chained (no device)


def chain_forward(x, params, spec, running=None):
    """The whole forward from the node references alone, every decision the references' own: x (B,H,W,cin) float64, params in plan
    order, running = [(mean, var)] * 12 for eval-mode BatchNorm.  Y / norm / A (activations) per block, P per level, S, y."""
    w, gamma, beta, wout = split_params(params)
    B = x.shape[0]
    r = SimpleNamespace(Y=[None] * NCONV, norm=[None] * NCONV, A=[None] * NCONV, P=[None] * NLEV, stats=[None] * NCONV, inp=[None] * NCONV)

    def block(i, inp):
        r.inp[i] = spec.q(inp)
        r.Y[i] = conv(r.inp[i], spec.q(w[i]))
        if spec.batch_stats:
            r.stats[i] = norm_stats(r.Y[i], spec)
            mean, var = r.stats[i][0], r.stats[i][1]
        else:
            mean, var = _per_sample(running[i][0].double(), B), _per_sample(running[i][1].double(), B)
        r.norm[i] = norm_arrays(mean, var, gamma[i], beta[i], spec.eps)
        r.A[i] = act(r.Y[i], r.norm[i][0], r.norm[i][1])
        return r.A[i]

    for k in range(NLEV):
        r.P[k] = x.detach().double() if k == 0 else pool(r.A[2 * k - 1])
        block(2 * k + 1, block(2 * k, r.P[k]))
    r.S = sum(upsample(r.A[2 * k + 1], 1 << k) for k in range(NLEV))
    block(11, block(10, r.S))
    r.y = conv(spec.q(r.A[11]), spec.q(wout))
    return r


def chain_backward(fw, params, spec, dy, dx_channels):
    """The whole backward from the node references, in the plan's order and with its intermediate buffers (dS, the x passes tx_k of
    the up-sampling adjoints, the composite dA of each level's second block), decisions taken from the forward `fw` of chain_forward."""
    w, gamma, beta, wout = split_params(params)
    r = SimpleNamespace(dA=[None] * NCONV, dY=[None] * NCONV, dW=[None] * NCONV, dgamma=[None] * NCONV, dbeta=[None] * NCONV,
                        k1=[None] * NCONV, k2=[None] * NCONV, TX=[None] * NLEV)

    def block(i, dA):
        sc, sh, mean, rstd = fw.norm[i]
        r.dA[i] = dA
        r.dgamma[i], r.dbeta[i], r.k1[i], r.k2[i], r.dY[i] = norm_bwd(dA, fw.Y[i], preact(fw.Y[i], sc, sh) > 0, mean, rstd, gamma[i], spec)
        r.dW[i] = conv_dw(fw.inp[i], spec.q(r.dY[i]))
        return conv_dx(spec.q(r.dY[i]), spec.q(w[i]))

    dy = dy.detach().double()
    r.dWout = conv_dw(spec.q(fw.A[11]), dy, 1)
    r.G0 = block(10, block(11, conv_dx(dy, spec.q(wout))))
    dP = None
    for k in range(NLEV - 1, -1, -1):
        r.TX[k] = up_adj_x(r.G0, 1 << k) if k else r.G0
        dA = up_adj_y(r.TX[k], 1 << k)
        if dP is not None:
            dA = dA + pool_route(fw.A[2 * k + 1], dP)
        dP = block(2 * k, block(2 * k + 1, dA))
    r.dx = dP[..., :dx_channels]
    return r
