"""
Node-level oracle of HalfUNet's module path in bf16 (py4cast_amd/halfunet.py: `_forward_modules`, the HalfUNetSettings combinations the
fused plan is not built for): a recorder of the native node calls of a forward / backward (ops_model.conv_nhwc, ops_ghost.ghost_dw),
float64 references of those nodes on the stored operands, the comparison with its bars, and the network-level helpers -- shared by
tests/test_halfunet_settings_bf16_gpu.py (the device) and tests/test_halfunet_settings_nodes_cpu.py (the references, the plumbing and the
sensitivity of the comparison, without a device).  Importing it needs no GPU.

Conventions.  Features-last (B, H, W, C) tensors.  The convolution kernels round the fp32 master weight to bf16 while staging it, so the
float64 convolution takes `w.bfloat16().double()` (tests/test_widen_gpu.py, the compact-convolution test); the depthwise kernels of
`ghost_dw` read the fp32 weight as it is (tests/test_round2_gpu.py::test_ghost_depthwise_kernels).
"""
import copy

import torch
import torch.nn.functional as F

CIN, COUT, B = 21, 12, 2
BF16 = {"compute_dtype": "bf16", "activation_dtype": "bf16"}
ROWS = {
    "nf32": dict(num_filters=32),
    "bias": dict(bias=True),
    "ghost-bias": dict(use_ghost=True, bias=True),
    "ghost-nf48": dict(use_ghost=True, num_filters=48),
    "group": dict(num_filters=32, norm="group", groups=4),
    "tanh": dict(last_activation="Tanh"),
}
# 48 x 80: levels 48x80, 24x40 (the row kernel's W > 32, H >= 8), 12x20, 6x10, 3x5 (not); 16 x 16: the coarsest level is 1 x 1
GRID = (48, 80)
CASES = [(row, *GRID) for row in ROWS] + [("nf32", 16, 16), ("ghost-bias", 16, 16)]
CASE_IDS = [f"{r}-{h}x{w}" for r, h, w in CASES]
# the seeds of test_halfunet_yaml_settings_match_oracle; at 16 x 16 the weights are drawn with seed 1 instead: with seed 19 the
# float64 problem itself is badly conditioned there for the Ghost row (batch norm over the two samples of a 1 x 1 map: the ORACLE run in
# fp32 is 7.9e-3 from itself in float64 in every gradient, 4e-5 with seed 1 -- tests/test_halfunet_settings_nodes_cpu.py asserts this
# conditioning, on the oracle alone, for every case)
SEED_MODEL, SEED_X, SEED_GY = {(48, 80): 19, (16, 16): 1}, 20, 21

# one bf16 rounding of an fp32 accumulation over exactly represented operands (tests/test_gemm_gpu.py): at most 2^-9 of each element
OUT_REL, OUT_MAX = 3e-3, 6e-3
WGRAD_REL = 2e-3            # fp32 weight gradients (the compact-convolution test)
GHOST_TOL = 8e-3            # test_ghost_depthwise_kernels in bf16: output, data gradient, and max(tol, 2e-5) for the weight gradient
ALIVE = 1e-6                # a node's reference results against the norm product of its operands


def pad32(c):
    return (c + 31) // 32 * 32


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def worst(got, ref):
    """largest deviation over the largest reference magnitude"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ models and inputs
def make_models(row, H, W, bf16=True, **extra):
    """(HalfUNetMI355X on the CPU, float64 oracle) on one state dict"""
    from oracle.halfunet import HalfUNetRef
    from py4cast_amd.halfunet import HalfUNetMI355X, HalfUNetSettings

    kw = ROWS[row]
    torch.manual_seed(SEED_MODEL.get((H, W), 19))
    model = HalfUNetMI355X(CIN, COUT, (H, W), HalfUNetSettings(**kw, **(BF16 if bf16 else {}), **extra))
    assert model.module_path and not model.ghost_native and model.native_rollout is None
    ref = HalfUNetRef(CIN, COUT, **kw).double()
    assert set(model.state_dict()) == set(ref.state_dict())
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()})
    return model, ref


def make_inputs(H, W):
    x = torch.randn(B, H, W, CIN, generator=torch.Generator().manual_seed(SEED_X))
    gy = torch.randn(B, H, W, COUT, generator=torch.Generator().manual_seed(SEED_GY))
    return x, gy


def level_of(H0, h):
    """0 .. 4: which level of an H0-row network a map of h rows belongs to"""
    k = {H0 >> i: i for i in range(5)}
    return k[h]


# ------------------------------------------------------------------------------------------------ the recorder
class Recorder:
    """While active, wraps `py4cast_amd.ops_model.conv_nhwc` and `py4cast_amd.ops_ghost.ghost_dw` -- the attributes halfunet.py looks
    up at call time -- and keeps per call clones of the operands (x, w) and of the stored output y, through tensor hooks the dy the
    output received and the dx handed back, and for conv_nhwc the route (`_compact_ok`) and the kernel kind `conv_kernel_kind` reports
    for the padded launch.  The calls themselves are untouched: the same arguments (x through a view of itself, so that its hook sees
    this call's gradient alone), the same kernels.  ``undo()`` restores everything.

    ``conv`` / ``ghost`` replace the two nodes (the CPU tests run the comparison on stand-ins, `emulated_conv_nhwc` / `emulated_ghost_dw`;
    `conv_nhwc_supported` then answers True, as it does for every convolution of these networks on the device)."""

    def __init__(self, conv=None, ghost=None, routes=True):
        from py4cast_amd import ops_ghost as OG
        from py4cast_amd import ops_model as OM

        self.OM, self.OG, self.routes = OM, OG, routes
        self.orig = {"conv_nhwc": OM.conv_nhwc, "ghost_dw": OG.ghost_dw, "conv_nhwc_supported": OM.conv_nhwc_supported}
        self.nodes = {"conv": conv or OM.conv_nhwc, "ghost": ghost or OG.ghost_dw}
        self.calls = []
        OM.conv_nhwc = lambda x, w: self._call("conv", x, w)
        OG.ghost_dw = lambda y, w: self._call("ghost", y, w)
        if conv is not None:
            OM.conv_nhwc_supported = lambda x, w: True

    def _call(self, kind, x, w):
        rec = {"kind": kind, "x": x.detach().clone(), "w": w.detach().clone(), "dy": None, "dx": None}
        if kind == "conv" and self.routes:
            Bn, H, W, _ = x.shape
            rec["compact"] = bool(self.OM._compact_ok(x, w))
            rec["kernel_kind"] = self.OM.conv_kernel_kind(Bn, H, W, pad32(w.shape[1]), w.shape[-1])
        xi = x.view_as(x) if x.requires_grad else x
        y = self.nodes[kind](xi, w)
        rec["y"] = y.detach().clone()
        if xi.requires_grad:
            xi.register_hook(lambda g: rec.__setitem__("dx", g.detach().clone()))
        if y.requires_grad:
            y.register_hook(lambda g: rec.__setitem__("dy", g.detach().clone()))
        self.calls.append(rec)
        return y

    def rerun(self, rec):
        """the node alone on the recorded operands and the recorded dy: (y, dx, dw)"""
        xl, wl = rec["x"].clone().requires_grad_(True), rec["w"].clone().requires_grad_(True)
        with torch.enable_grad():
            y = self.nodes[rec["kind"]](xl, wl)
            y.backward(rec["dy"])
        return y.detach(), xl.grad, wl.grad

    def undo(self):
        self.OM.conv_nhwc, self.OM.conv_nhwc_supported = self.orig["conv_nhwc"], self.orig["conv_nhwc_supported"]
        self.OG.ghost_dw = self.orig["ghost_dw"]


def library_route(monkeypatch):
    """`ops_model.conv_nhwc_supported` answers False: `_conv_module` and `_ghost_module` take their F.conv2d branches -- the same
    network, the same bf16 stored maps, torch's kernels.  The reference route of the network-level bars; nothing in the product changes."""
    from py4cast_amd import ops_model as OM

    monkeypatch.setattr(OM, "conv_nhwc_supported", lambda x, w: False)


def run_recorded(model, x, gy, forward=None, **kw):
    """one training forward + backward under a Recorder (`forward`: the model itself on the device, `_forward_modules` on the CPU, where
    forward() refuses tensors): (recorder, y, dx, parameter gradients by name)"""
    model.train()
    model.zero_grad(set_to_none=True)
    rec = Recorder(**kw)
    try:
        xg = x.clone().requires_grad_(True)
        y = (forward or model._forward_modules)(xg)
        y.backward(gy)
    finally:
        rec.undo()
    return rec, y.detach(), xg.grad, {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def expected_kernel_kind(H, W, cp, ks):
    """p4c_conv_kernel_kind for a bf16 (B <= 32, H, W, cp) map as csrc/conv_rows.hip::conv_bf16_is_rows and csrc/conv_bf16.hip::
    is_tile_ring decide it: both serve 64 input channels only; rows (2) for W > 32 and H >= 8 at ks 1 or 3, the tile ring (1) for
    every other 3x3, the generic tile kernel (0) for the rest"""
    if cp == 64 and W > 32 and H >= 8:
        return 2
    return 1 if cp == 64 and ks == 3 else 0


def check_routes(rec, row, H0, W0):
    """The route facts of a recording, per conv_nhwc call.  The compact route (`_compact_ok`) is taken exactly where the map has
    C = CI and both channel counts are multiples of 8 below 64 x 64 AND the level satisfies the row kernel's W > 32, H >= 8 (48 x 80:
    levels 0 and 1); never below 24 x 40 and nowhere on a 16 x 16 grid.  The padded launches' kernel kinds are the ones the dispatch
    code gives for their shapes; the rows with 64-channel (padded) inputs meet all of 2, 1 and 0 at 48 x 80.  Returns the kinds met."""
    convs = [r for r in rec.calls if r["kind"] == "conv"]
    assert convs
    kinds, ncompact = set(), 0
    for r in convs:
        _, H, W, C = r["x"].shape
        CO, CI, ks, _ = r["w"].shape
        tag = f"{row} {H0}x{W0}: conv {CI}->{CO} ks {ks} at {H}x{W}"
        wide = W > 32 and H >= 8
        assert wide == (level_of(H0, H) < 2 and (H0, W0) == GRID), tag
        want_compact = wide and C == CI and C % 8 == 0 and CO % 8 == 0 and (C < 64 or CO < 64)
        assert r["compact"] == want_compact, f"{tag}: compact route {r['compact']}"
        if not wide:
            assert not r["compact"], tag
        assert r["kernel_kind"] == expected_kernel_kind(H, W, pad32(CI), ks), f"{tag}: kernel kind {r['kernel_kind']}"
        if r["compact"]:
            ncompact += 1
        else:
            kinds.add(r["kernel_kind"])
    if (H0, W0) == GRID:
        if row in ("nf32", "group"):
            # enc1conv2, enc2conv1, enc2conv2, decoderconv1, decoderconv2: 32 -> 32 on the row kernel; 21 -> 32 and 32 -> 12 padded
            assert ncompact == 5 and kinds == {0}, (row, ncompact, kinds)
        elif row == "ghost-nf48":
            assert ncompact == 5 and kinds == {0, 1, 2}, (row, ncompact, kinds)          # 48 -> 24 compact; 48 -> 64 padded below
        else:
            assert ncompact == 0 and kinds == {0, 1, 2}, (row, ncompact, kinds)          # 64 -> 64: rows, ring, and 21 -> 32 generic
    else:
        assert ncompact == 0
    return kinds


# ------------------------------------------------------------------------------------------------ float64 node references
def conv_ref(x, w, dy, groups=1, round_weight=True):
    """"same" convolution in float64 on the stored operands, the weight rounded to bf16 as the kernels stage it: (y, dx, dw)"""
    x64 = x.detach().cpu().double().permute(0, 3, 1, 2).requires_grad_(True)
    wd = w.detach().cpu()
    w64 = (wd.bfloat16() if round_weight else wd).double().requires_grad_(True)
    with torch.enable_grad():
        y = F.conv2d(x64, w64, padding=w.shape[-1] // 2, groups=groups)
        dx, dw = torch.autograd.grad(y, [x64, w64], dy.detach().cpu().double().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1), dw


def ghost_ref(y, w, dout):
    """[prim | depthwise3x3(prim)] of the 32 primary channels of a 64-channel map, float64, the fp32 weight as it is: (out, dy, dw)"""
    y64 = y.detach().cpu().double().requires_grad_(True)
    w64 = w.detach().cpu().double().requires_grad_(True)
    with torch.enable_grad():
        prim = y64[..., :32]
        out = torch.cat([prim, F.conv2d(prim.permute(0, 3, 1, 2), w64, padding=1, groups=32).permute(0, 2, 3, 1)], dim=-1)
        dy, dw = torch.autograd.grad(out, [y64, w64], dout.detach().cpu().double())
    return out.detach(), dy, dw


def node_ref(rec, w=None):
    """the float64 reference of a recorded call (`w`: another weight than the recorded one -- the sensitivity tests)"""
    w = rec["w"] if w is None else w
    return conv_ref(rec["x"], w, rec["dy"]) if rec["kind"] == "conv" else ghost_ref(rec["x"], w, rec["dy"])


def alive(rec, ref):
    """each reference result over the norm product of its operands (the CPU test asserts > ALIVE for every node)"""
    n = lambda t: float(t.detach().double().norm())
    yr, dxr, dwr = ref
    x, w, dy = n(rec["x"]), n(rec["w"]), n(rec["dy"])
    return {"y": n(yr) / max(x * w, 1e-300), "dx": n(dxr) / max(dy * w, 1e-300), "dw": n(dwr) / max(x * dy, 1e-300)}


def node_figures(rec, got, ref):
    """(figure, bar) per checked quantity of one node: got = (y, dx, dw) of the native node, ref = the float64 results"""
    y, dx, dw = got
    yr, dxr, dwr = ref
    if rec["kind"] == "conv":
        return {"y rel": (rel(y, yr), OUT_REL), "y max": (worst(y, yr), OUT_MAX), "dx rel": (rel(dx, dxr), OUT_REL),
                "dx max": (worst(dx, dxr), OUT_MAX), "dw rel": (rel(dw, dwr), WGRAD_REL)}
    return {"y rel": (rel(y, yr), GHOST_TOL), "dx rel": (rel(dx, dxr), GHOST_TOL), "dw rel": (rel(dw, dwr), max(GHOST_TOL, 2e-5))}


def check_nodes(rec, what, verbose=True):
    """Every recorded call against float64.  The node is run again on the recorded operands (that call's weight gradient alone): its
    output and data gradient must be the recorded ones bit for bit.  Returns the worst figure / bar ratio of the whole recording."""
    assert rec.calls, what
    top = 0.0
    for i, r in enumerate(rec.calls):
        tag = f"{what}: {r['kind']} call {i} x{tuple(r['x'].shape)} w{tuple(r['w'].shape)}"
        assert r["dy"] is not None and r["dx"] is not None, f"{tag}: no gradient recorded"
        y2, dx2, dw2 = rec.rerun(r)
        assert torch.equal(y2, r["y"]), f"{tag}: the re-run output differs from the recorded one"
        assert torch.equal(dx2, r["dx"]), f"{tag}: the re-run data gradient differs from the recorded one"
        assert r["dx"].shape == r["x"].shape and r["dx"].dtype == r["x"].dtype, tag      # nothing beyond the real input channels
        assert dw2.shape == r["w"].shape and dw2.dtype == torch.float32, tag
        for t in (r["y"], r["dx"], dw2):
            assert bool(torch.isfinite(t.float()).all()), tag
        if r["kind"] == "ghost":
            assert torch.equal(r["y"][..., :32], r["x"][..., :32]), f"{tag}: the primary half is not a copy"
            assert float(r["dx"][..., 32:].float().abs().sum()) == 0.0, f"{tag}: gradient in the ignored channels 32..63"
        figs = node_figures(r, (r["y"], r["dx"], dw2), node_ref(r))
        if verbose:
            route = "" if "compact" not in r else f" [{'compact' if r['compact'] else 'padded, kind %d' % r['kernel_kind']}]"
            print(f"{tag}{route}: " + " ".join(f"{k} {v:.2e}" for k, (v, _) in figs.items()))
        for k, (v, bar) in figs.items():
            assert v <= bar, f"{tag}: {k} {v:.3e} > {bar:.1e}"
            top = max(top, v / bar)
    return top


# ------------------------------------------------------------------------------------------------ stand-ins of the two nodes (CPU)
def _bf16_weight(w):
    """the bf16 image of w in the forward, the identity in the backward (the kernels' weight gradient is fp32)"""
    return w + (w.detach().bfloat16().to(w.dtype) - w.detach())


def emulated_conv_nhwc(x, w, prepare=_bf16_weight):
    """what `conv_nhwc` computes, with torch on any device: fp32 accumulation over the stored operands and the bf16 image of the weight,
    one rounding to the map's dtype, an fp32 weight gradient"""
    y = F.conv2d(x.float().permute(0, 3, 1, 2), prepare(w.float()), padding=w.shape[-1] // 2)
    return y.permute(0, 2, 3, 1).to(x.dtype)


def emulated_ghost_dw(y, w):
    prim = y[..., :32]
    cheap = F.conv2d(prim.float().permute(0, 3, 1, 2), w.float(), padding=1, groups=32).permute(0, 2, 3, 1).to(y.dtype)
    return torch.cat([prim, cheap], dim=-1)


def swap_taps(w, a=(0, 0), b=(0, 1)):
    """w with two taps of its 3x3 window exchanged (a wrong tap in a kernel)"""
    out = w.clone()
    out[..., a[0], a[1]], out[..., b[0], b[1]] = w[..., b[0], b[1]], w[..., a[0], a[1]]
    return out


# ------------------------------------------------------------------------------------------------ the network against the oracle
QUANTITIES = ("output", "input gradient", "parameter gradients", "running statistics", "eval output")


def train_then_eval(model, x, gy, dev, forward=None):
    """the five quantities of tests/test_ghost_native_gpu.py::train_then_eval, and the parameter gradients by name"""
    forward = forward or model
    model.train()
    model.zero_grad(set_to_none=True)
    xg = x.detach().clone().to(dev).requires_grad_(True)
    y = forward(xg)
    y.backward(gy.to(dev))
    named = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}
    grads = torch.cat([named[n].reshape(-1) for n in sorted(named)])
    stats = [b.detach().double().reshape(-1).cpu() for _, b in sorted(model.named_buffers()) if b.dtype.is_floating_point]
    model.eval()
    with torch.no_grad():
        ye = forward(x.to(dev))
    model.train()
    return {"output": y.detach(), "input gradient": xg.grad, "parameter gradients": grads,
            "running statistics": torch.cat(stats) if stats else None, "eval output": ye, "named": named}


def oracle_train_then_eval(ref, x, gy, dtype=torch.float64):
    ref = copy.deepcopy(ref).to(dtype)
    ref.train()
    xr = x.detach().to(dtype).requires_grad_(True)
    yr = ref(xr.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    yr.backward(gy.to(dtype))
    named = {n: p.grad.detach() for n, p in ref.named_parameters()}
    grads = torch.cat([named[n].reshape(-1) for n in sorted(named)])
    stats = [b.reshape(-1).double() for _, b in sorted(ref.named_buffers()) if b.dtype.is_floating_point]
    ref.eval()
    with torch.no_grad():
        ye = ref(x.to(dtype).permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    return {"output": yr.detach(), "input gradient": xr.grad, "parameter gradients": grads,
            "running statistics": torch.cat(stats) if stats else None, "eval output": ye, "named": named}


def conv_biases(named):
    """the convolution biases of a gradient dict (not the norms' shifts)"""
    return [n for n in sorted(named) if n.endswith(".bias") and "conv" in n.split(".")[-2]]


def bias_distance(got, want, name):
    """|got - want| of a bias gradient over max(|want|, 1e-2 |its layer's weight gradient|): a convolution bias in front of a batch
    norm has a true gradient of zero (test_halfunet_yaml_settings_match_oracle), so it is judged against its layer's weight gradient"""
    g, r = got[name].double(), want[name].double()
    scale = max(float(r.norm()), 1e-2 * float(want[name[:-4] + "weight"].double().norm()))
    return float((g - r).norm()) / scale
