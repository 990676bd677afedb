"""
TEST INFRASTRUCTURE ONLY.  Float64 references of the streaming kernels of csrc/losses.hip and csrc/rollout.hip, and the launch
arithmetic of those kernels restated in Python (tests/test_step_reference_cpu.py proves both; tests/test_loop_trips_gpu.py uses them).

Layout: the graph layout of the C ABI -- prediction / target / mask (B, T, N, F), states (B, N, F), network rows (B, N, y_cs),
interior / border masks flat (N,).  The references are plain torch on whatever device their operands live on; they convert to
``dtype`` (float64 by default) first and gradients come from autograd.  The element references (``ar_update``, ``build_x``,
``unnormalize``) keep the kernels' operation order, so with ``dtype=torch.float32`` they are the fp32 torch chain the kernels equal
bit for bit (every torch op rounds once; the kernels are compiled without FMA contraction).
"""
import torch

MASK_MODES = ("none", "from_nan", "f32", "u8")   # p4c_mask_mode 0..3
KINDS = ("mse", "l1")                            # p4c_loss_kind 0, 1


# ------------------------------------------------------------------------------------------------ losses
def resolve_mask(target, mode="none", mask=None, dtype=torch.float64):
    """(mask, target) as the kernels' load_mask sees them (losses.hip:34-45): FROM_NAN masks the NaN elements of the target and
    replaces them by 0; F32 multiplies by the mask's value; U8 by 1 where the byte is set."""
    t = target.to(dtype)
    if mode == "none":
        return torch.ones_like(t), t
    if mode == "from_nan":
        return (~torch.isnan(t)).to(dtype), torch.nan_to_num(t, nan=0.0)
    if mode == "f32":
        return mask.to(dtype), t
    if mode == "u8":
        return (mask != 0).to(dtype), t
    raise KeyError(mode)


def _elem(pred, tgt, m, kind):
    d = pred * m - tgt * m                                       # losses.py:144 / 195
    return d * d if kind == "mse" else d.abs()


def masked_count(target, mode="none", mask=None):
    """Number of grid points whose mask is zero for EVERY (b, t, f) -- border points included (losses.py:156, 167)."""
    m, _ = resolve_mask(target, mode, mask)
    return int((~(m != 0).any(dim=3).any(dim=1).any(dim=0)).sum())


def weighted_loss_map(pred, target, weights, kind="mse", mode="none", mask=None, dtype=torch.float64):
    """losses.py:144-150 -> (B, T, N)."""
    m, t = resolve_mask(target, mode, mask, dtype)
    return (_elem(pred.to(dtype), t, m, kind) * weights.to(dtype)).sum(-1)


def weighted_loss(pred, target, weights, interior, kind="mse", mode="none", mask=None, dtype=torch.float64):
    """losses.py:130-169 -> (B, T)."""
    wl = weighted_loss_map(pred, target, weights, kind, mode, mask, dtype)
    denom = float(interior.sum()) - masked_count(target, mode, mask)
    return (wl * interior.to(dtype)).sum(-1) / denom


def scaled_loss(pred, target, std, interior, kind="mse", mode="none", mask=None, dtype=torch.float64):
    """losses.py:186-210 -> (B, T, F)."""
    m, t = resolve_mask(target, mode, mask, dtype)
    e = _elem(pred.to(dtype), t, m, kind)
    denom = float(interior.sum()) - masked_count(target, mode, mask)
    v = (e * interior.to(dtype)[:, None]).sum(2) / denom
    if kind == "mse":
        v = v.sqrt()
    return v * std.to(dtype)


def acc_sums(pred, target, climate_means, mode="none", mask=None, dtype=torch.float64):
    """MetricACC.update (metrics.py:414-423) -> (3, B, T, F): spatial means of (p-c)(t-c)m, ((p-c)m)^2, ((t-c)m)^2."""
    m, t = resolve_mask(target, mode, mask, dtype)
    c = climate_means.to(dtype)
    dp, dt = pred.to(dtype) - c, t - c
    return torch.stack([(dp * dt * m).mean(2), ((dp * m) ** 2).mean(2), ((dt * m) ** 2).mean(2)])


def nan_moments(x, x_next=None, dtype=torch.float64):
    """compute_dataset_stats.py:45-52, 105-108 -> (5, B, F): sum, sum of squares, count, min, max of the non-NaN values of x
    (or of x_next - x, the difference formed in the operands' own precision as the kernel forms it) over all rows of a sample."""
    v = (x_next - x if x_next is not None else x).to(dtype)
    B, F = v.shape[0], v.shape[-1]
    v = v.reshape(B, -1, F)
    ok = ~torch.isnan(v)
    z = torch.where(ok, v, torch.zeros_like(v))
    mn = torch.nan_to_num(v, nan=float("inf")).min(dim=1).values
    mx = torch.nan_to_num(v, nan=float("-inf")).max(dim=1).values
    return torch.stack([z.sum(1), (z * z).sum(1), ok.sum(1).to(dtype), mn, mx])


# ------------------------------------------------------------------------------------------------ element kernels
def ar_update(prev, y, border_state=None, std=None, mean=None, border_mask=None, interior_mask=None, keep_prev=1.0,
              nan_to_num=False, dtype=torch.float64):
    """lightning.py:599-633 in the kernels' operation order (rollout.hip ar_update_fwd_kernel, losses.hip:586-593):
    p * keep + y * std, + mean, then border * border_state + interior * predicted."""
    if prev is not None:
        F = prev.shape[-1]
    elif border_state is not None:
        F = border_state.shape[-1]
    else:
        F = std.numel() if std is not None else y.shape[-1]
    yv = y[..., :F].to(dtype)
    p = torch.zeros_like(yv) if prev is None else prev.to(dtype)
    if nan_to_num:
        p = torch.nan_to_num(p, nan=0.0)
    if std is not None:
        pr = p * keep_prev + yv * std.to(dtype)
        pr = pr + mean.to(dtype)
    else:
        pr = p * keep_prev + yv
    if border_mask is not None:
        bs = border_state.to(dtype)
        if nan_to_num:
            bs = torch.nan_to_num(bs, nan=0.0)
        pr = border_mask.to(dtype)[:, None] * bs + interior_mask.to(dtype)[:, None] * pr
    return pr


def build_x(prev_states, statics, forcing, c_pad=None, out_dtype=torch.float32, mask_on_nan=False):
    """lightning.py:711-767: prev_states (B, T_in, N, F), statics (B, N, Fs), forcing (B, N, Ff) -> (B, N, c_pad) in ``out_dtype``:
    the input steps, statics, forcing, the optional "no NaN anywhere" channel, zero padding.  A copy and a conversion per element."""
    B, T_in, N, F = prev_states.shape
    parts = [prev_states[:, t] for t in range(T_in)]
    tail = []
    if mask_on_nan:
        bad = torch.isnan(forcing).any(-1)
        for p in parts:
            bad = bad | torch.isnan(p).any(-1)
        tail = [(~bad).unsqueeze(-1).to(prev_states.dtype)]
        parts = [torch.nan_to_num(p, nan=0.0) for p in parts]
        forcing = torch.nan_to_num(forcing, nan=0.0)
    x = torch.cat(parts + [statics, forcing] + tail, dim=-1)
    if c_pad is not None and c_pad > x.shape[-1]:
        x = torch.cat([x, torch.zeros(B, N, c_pad - x.shape[-1], dtype=x.dtype, device=x.device)], dim=-1)
    return x.to(out_dtype)


def unnormalize(x, std, mean, dtype=torch.float64):
    """lightning.py:1162-1169: two rounded steps, x * std then + mean."""
    v = x.to(dtype) * std.to(dtype)
    return v + mean.to(dtype)


# ------------------------------------------------------------------------------------------------ the fused AR step
def fused_step(prev, y, target, std, mean, border_mask, interior_mask, weights, kind="mse", keep_prev=1.0, from_nan=False,
               loss=True, next_input=None, state=None, dtype=torch.float64):
    """One AR step as the fused kernels compute it (losses.hip:555-604): state update (scaled when ``std`` is given), border
    forcing (when ``border_mask`` is given), that step's weighted-loss column, the next network input and the saved loss gradient.

    prev (B, N, F) or None, y (B, N, y_cs), target (B, N, F) (None for a free step that forces nothing).  ``loss=False`` is the free
    step: no loss column, no saved gradient.  ``next_input`` = (statics, forcing, c_pad, dtype) asks for the next input.
    ``state``: the new state a kernel stored in fp32; the loss terms are then evaluated AT that state (the operand the kernels'
    backward reads) while gradients still flow through the update -- a straight-through substitution.
    Returns a dict: new_state (B, N, F), loss (B,) or None, x_next or None, lgrad (B, N, F) = d loss_elem / d pred or None.
    Tensors that require grad keep their graph: see ``fused_step_grads``."""
    mode = "from_nan" if from_nan else "none"
    F = (target if target is not None else prev).shape[-1]
    m = t = None
    if target is not None:
        m, t = resolve_mask(target, mode, None, dtype)
    yv = y[..., :F].to(dtype)
    p = torch.zeros_like(yv) if prev is None else prev.to(dtype)
    if from_nan:
        p = torch.nan_to_num(p, nan=0.0)
    if std is not None:
        pr = p * keep_prev + yv * std.to(dtype)
        pr = pr + mean.to(dtype)
    else:
        pr = p * keep_prev + yv
    im = None if interior_mask is None else interior_mask.to(dtype)[:, None]
    if border_mask is not None:
        pr = border_mask.to(dtype)[:, None] * t + im * pr
    ns = pr
    if state is not None:
        ns = pr + (state.to(dtype) - pr).detach()
    out = {"new_state": ns, "loss": None, "x_next": None, "lgrad": None}
    if loss:
        denom = float(interior_mask.sum()) - masked_count(target.unsqueeze(1), mode)
        e = _elem(ns, t, m, kind)
        out["loss"] = ((e * weights.to(dtype)).sum(-1) * im[:, 0]).sum(-1) / denom
        d = (ns * m - t * m).detach()
        out["lgrad"] = (2.0 * d if kind == "mse" else torch.sign(d)) * m
        out["denom"] = denom
    if next_input is not None:
        statics, forcing, c_pad, xdt = next_input
        src = ns.detach() if state is None else state.to(dtype)
        out["x_next"] = build_x(src.unsqueeze(1), statics.to(dtype), forcing.to(dtype), c_pad, xdt)
    return out


def fused_step_grads(out, y, prev, gloss=None, g_next=None, g_next2=None, interior_mask=None, weights=None, lgrad=None):
    """(dy, dprev) of a ``fused_step`` result by torch.autograd.grad: the objective is sum(gloss * loss) + sum((g_next + g_next2[...,
    :F]) * new_state), i.e. both upstream gradients arrive at the new state (losses.hip:665-669).  ``y`` / ``prev`` are the float64
    leaves the step was built from (dy has y's channel count: channels >= F come out zero).  ``lgrad``: evaluate the loss term from
    SAVED loss gradients (the bf16 rows of p4c_ar_update_loss_fwd_next_saved) instead -- sum(gloss / denom * interior * w * lgrad *
    new_state), linear in the state."""
    ns = out["new_state"]
    F = ns.shape[-1]
    obj = ns.new_zeros(())
    if gloss is not None:
        if lgrad is not None:
            coef = (gloss.to(ns.dtype) / out["denom"])[:, None, None] * interior_mask.to(ns.dtype)[None, :, None] * weights.to(ns.dtype)
            obj = obj + (coef * lgrad.to(ns.dtype) * ns).sum()
        else:
            obj = obj + (gloss.to(ns.dtype) * out["loss"]).sum()
    if g_next is not None:
        obj = obj + (g_next.to(ns.dtype) * ns).sum()
    if g_next2 is not None:
        obj = obj + (g_next2[..., :F].to(ns.dtype) * ns).sum()
    leaves = [y] + ([prev] if prev is not None else [])
    grads = torch.autograd.grad(obj, leaves, allow_unused=True)
    dy = grads[0] if grads[0] is not None else torch.zeros_like(y)
    dprev = None
    if prev is not None:
        dprev = grads[1] if grads[1] is not None else torch.zeros_like(prev)
    return dy, dprev


# ------------------------------------------------------------------------------------------------ launch arithmetic
LOSS_MAX_BLOCKS = 512      # losses.hip:26
FLAT_P = 64                # losses.hip:686 (and BX_P, rollout.hip:317)
WAVES_PER_BLOCK = 4        # 256 threads


def _cdiv(a, b):
    return -(-a // b)


def pow2_ge64(v):
    """losses.hip:19-23 (pow2_ge64) and rollout.hip:19-23 (pow2_ge): the smallest power of two >= v, at most 64."""
    p = 1
    while p < v and p < 64:
        p <<= 1
    return p


def loss_blocks(N, PP, nbt, cus):
    """losses.hip:1144-1154: blocks per (b, t) of a loss kernel whose waves take PP grid points per pass."""
    blocks = _cdiv(_cdiv(N, PP), WAVES_PER_BLOCK)
    cap = max(_cdiv(cus * 8, nbt), 1)
    return max(min(blocks, cap, LOSS_MAX_BLOCKS), 1)


def stream_grid(total, PP, cus):
    """rollout.hip:369-377: blocks of an element kernel over ``total`` rows, PP rows per wave and pass."""
    return max(min(_cdiv(_cdiv(total, PP), WAVES_PER_BLOCK), cus * 8), 1)


def flat_blocks(N, B, cus):
    """losses.hip:1391-1395: blocks per sample of a flat AR-step kernel (each walks tiles of FLAT_P grid points)."""
    return min(loss_blocks(N, FLAT_P // 4, B, cus), _cdiv(N, FLAT_P))


def trips(work, per_owner, owners):
    """The largest number of passes any owner (a wave, or the block that owns a tile) makes through its grid-stride loop: ``work``
    items, ``per_owner`` of them per owner and pass, ``owners`` owners striding together."""
    return _cdiv(_cdiv(work, per_owner), owners)


def loss_trips(N, F, nbt, cus):
    """The stand-alone loss kernels, acc_sums' scalar form and nan_moments (losses.hip:1203-1204, 1291-1292, 1310-1311)."""
    PP = 64 // pow2_ge64(F)
    return trips(N, PP, WAVES_PER_BLOCK * loss_blocks(N, PP, nbt, cus))


def acc_v4_trips(N, F, nbt, cus):
    """acc_sums' 16-byte form (losses.hip:1285-1286)."""
    PP = 64 // pow2_ge64(F // 4)
    return trips(N, PP, WAVES_PER_BLOCK * loss_blocks(N, PP, nbt, cus))


def mask_count_blocks(N, F, cus):
    """losses.hip:1183-1186."""
    return max(min(_cdiv(_cdiv(N, 64 // pow2_ge64(F)), WAVES_PER_BLOCK), cus * 8), 1)


def mask_count_trips(N, F, cus):
    return trips(N, 64 // pow2_ge64(F), WAVES_PER_BLOCK * mask_count_blocks(N, F, cus))


def step_v4_trips(N, width, B, cus):
    """The 16-byte fused step: ``width`` = F forward (losses.hip:1411-1412), y_cs backward (losses.hip:1891-1892)."""
    PP = 64 // pow2_ge64(width // 4)
    return trips(N, PP, WAVES_PER_BLOCK * loss_blocks(N, PP, B, cus))


def step_scalar_trips(N, width, B, cus):
    """The scalar fused step: ``width`` = F forward (losses.hip:1446-1447), y_cs backward (losses.hip:1932-1934)."""
    return loss_trips(N, width, B, cus)


def step_flat_trips(N, B, cus):
    """The flat fused step, forward and backward (losses.hip:789, 965, 1426, 1911): tiles per block."""
    return trips(N, FLAT_P, flat_blocks(N, B, cus))


def row_stream_trips(rows, width, cus):
    """ar_update fwd (width = F, rollout.hip:727-729) / bwd (y_cs, :749-751), build_x's scalar kernel (c_pad, :393, 450) and
    build_x_bwd (T_in * F, :644-646): ``rows`` = B * N rows over one grid."""
    PP = 64 // pow2_ge64(width)
    return trips(rows, PP, WAVES_PER_BLOCK * stream_grid(rows, PP, cus))


def build_x_v4_trips(N, c_pad, cus):
    """build_x's 16-byte kernel: one grid of stream_grid(N, ..) blocks per sample (rollout.hip:429, 434)."""
    PP = 64 // pow2_ge64((c_pad + 3) // 4)
    return trips(N, PP, WAVES_PER_BLOCK * stream_grid(N, PP, cus))


def build_x_flat_trips(N, B, cus):
    """build_x's flat kernel (rollout.hip:409-412): tiles of 64 grid points over 8 * CUs / B blocks per sample."""
    ntiles = _cdiv(N, FLAT_P)
    return _cdiv(ntiles, max(min(cus * 8 // max(B, 1), ntiles), 1))


def unnormalize_trips(rows, F, cus):
    """p4c_unnormalize (rollout.hip:578-581): one element per thread, at most 16 * CUs blocks of 256."""
    total = rows * F
    return _cdiv(total, 256 * min(_cdiv(total, 256), cus * 16))


def sum_state_grads_trips(B, N, F, cus):
    """p4c_sum_state_grads (rollout.hip:685, 711): one element per lane."""
    total = B * N * F
    return trips(total, 64, WAVES_PER_BLOCK * stream_grid(total, 64, cus))
