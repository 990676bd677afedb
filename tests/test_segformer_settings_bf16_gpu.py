"""
Segformer's non-default settings on the bf16 route: four configurations (tests/segformer_settings_cases.py) that take the kernels off the
default widths -- FFN widths 32 / 64 / 96, dims up to 512 with 16 heads, reduction ratios 1 and 16, key counts with a masked tail (2, 3, 8,
12), whole chunks (192) and the cap (256), one and three layers, decoder_dim 64 / 128, 8- and 64-channel downsamplers -- each checked
NODE BY NODE against float64 on the operands recorded in one forward / backward (tests/segformer_nodes.py):

* LayerNorm, attention core and the two block kinds: the checks and bars of tests/test_segformer_nodes_gpu.py, imported;
* the nodes outside the blocks -- downsampler, the four patch embeddings, the four decoder pairs, up_sum, the head and its x8 bilinear
  up-sampling: each stores ONE bf16 result of an fp32 accumulation over bf16 operands, so the kernel bars of tests/test_gemm_gpu.py hold
  (6e-3 of the largest magnitude, 3e-3 in the 2-norm), forward and data gradient; their fp32 parameter gradients (taken from the
  network's own backward: every one of these parameters has exactly one consumer) 5e-3 as test_patch_conv_against_float64;
* the decoder's weight slices: the operands recorded are exactly columns [i dd, (i + 1) dd) of to_segmentation.0.weight, the bias goes to
  stage 0 alone, and the up_sum output is the float64 Conv2d(4 dd, dd, 1) of the concatenated up-sampled stage maps;
* the chain: every recorded node's input is bit for bit the output of the node that feeds it in _forward_native, from the input rows
  to the returned tensor.  Every node checked and the chain exact: no whole-network bf16 bar is needed for these configurations.
The f32 flavour of each configuration runs against the float64 restatement built with the same settings at the fp32 bar 1e-4.
Once, on `narrow`: the pre-filled .grad / FlatDDP route and a bit-identical rerun.  The refusals: more than 256 keys.
Measured on an MI355X (profiles/segformer_settings_bf16.txt): every configuration passes as it stands.  One-rounding nodes 1.5e-3 ...
1.8e-3 in the 2-norm, the patch convolutions' dx 2.4e-3 (two roundings), the decoder figure 2.3e-3 ... 2.4e-3, fp32 parameter gradients
1e-7; of the block checks the Mix-FFN's dx - dy is the closest to its bar (2.2e-2 ... 3.0e-2 of 3e-2; fixed seeds and fixed-order sums).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import segformer_nodes as N  # noqa: E402
import segformer_reference as R  # noqa: E402
import segformer_settings_cases as C  # noqa: E402
import test_segformer_nodes_gpu as T  # noqa: E402  (its checks and bars: check_*_nodes, check_sink_route, close_bf16, rel)

pytestmark = pytest.mark.gpu

PARAM_BAR = 5e-3      # fp32 weight / bias sums of bf16 operands (tests/test_segformer_gpu.py::test_patch_conv_against_float64)
FP32_BAR = 1e-4       # the f32 flavour against float64 (tests/test_segformer_gpu.py::test_network_against_restatement)


def _inputs(name, dev):
    x, dy = C.make_inputs(name, dev)
    return x.to(torch.bfloat16), dy


@pytest.fixture(scope="module", params=C.NAMES)
def cfg(request, gpu_device):
    C.assert_case_shapes(request.param)
    name, dev = request.param, gpu_device
    m = C.make_model(name, "bf16", dev)
    C.assert_case_shapes(name, m)
    x, dy = _inputs(name, dev)
    rec = N.Recorder(m)
    try:
        y = m(x)
        y.float().backward(dy)
    finally:
        rec.undo()
    torch.cuda.synchronize()
    L = C.CASES[name]["num_layers"]
    assert len(rec.blocks) == 8 * L and len(rec.norms) == 8 * L and len(rec.attns) == 4 * L
    assert len(rec.patch_convs) == 5 and len(rec.linears) == 9 and len(rec.up_sums) == 1 and len(rec.upsamples) == 1
    assert all(r["dy"] is not None for r in rec.blocks + rec.patch_convs + rec.linears + rec.up_sums + rec.upsamples)
    assert tuple(r["kv"].shape[1] for r in rec.attns[::L]) == C.CASES[name]["keys"]
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    return {"name": name, "m": m, "rec": rec, "x": x, "y": y.detach(), "grads": grads, "layers": L}


# ------------------------------------------------------------------------------------------------ the present node checks
def test_layer_norm_and_attention_core_nodes(cfg):
    T.check_layer_norm_nodes(cfg["rec"])
    T.check_sra_core_nodes(cfg["rec"])


@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_block_nodes(cfg, kind):
    """with the condition that a block's own part is at least 0.05 of its input (asserted inside; the seeds make it hold:
    tests/test_segformer_settings_cpu.py)"""
    T.check_block_nodes(cfg["m"], cfg["rec"], kind, 4 * cfg["layers"])


# ------------------------------------------------------------------------------------------------ the nodes outside the blocks
def _params_of():
    """per recorded call outside the blocks, in call order: (weight parameter name, bias parameter name or None)"""
    convs = [("downsampler.weight", "downsampler.bias")] + [(f"mit.stages.{s}.1.weight", f"mit.stages.{s}.1.bias") for s in range(4)]
    lins = []
    for i in range(4):
        lins += [(f"to_fused.{i}.0.weight", f"to_fused.{i}.0.bias"), ("to_segmentation.0.weight", "to_segmentation.0.bias" if i == 0 else None)]
    lins.append(("to_segmentation.1.weight", "to_segmentation.1.bias"))
    return convs, lins


def _node_against_float64(what, run, ref, x, w, b, dy):
    """forward, data gradient (the native node alone on the recorded operands: the same output bit for bit, then dx for the recorded dy)
    against float64; returns (y, float64 dw, float64 db): the caller compares the network's own parameter gradients with these"""
    xl = x.clone().requires_grad_(True)
    y = run(xl, w, b)
    y.backward(dy)
    x64 = x.double().requires_grad_(True)
    leaves = [N._gemm_w(w).requires_grad_(True)] + ([] if b is None else [b.double().requires_grad_(True)])
    with torch.enable_grad():
        yr = ref(x64, leaves[0], None if b is None else leaves[1])
        grads = torch.autograd.grad(yr, [x64] + leaves, dy.double())
    T.close_bf16(y, yr, f"{what}: y")
    T.close_bf16(xl.grad, grads[0], f"{what}: dx")
    return y.detach(), grads[1], (None if b is None else grads[2])


def test_nodes_outside_the_blocks(cfg):
    from py4cast_amd import ops_gemm as G
    from py4cast_amd import segformer as S

    m, rec, got = cfg["m"], cfg["rec"], cfg["grads"]
    cin, O = m.in_channels, m.out_channels
    dd = m.to_segmentation[0].out_channels
    convs, lins = _params_of()
    params = dict(m.named_parameters())
    for i, (r, (wn, bn)) in enumerate(zip(rec.patch_convs, convs)):
        k, st, p = r["k"], r["stride"], r["pad"]
        what = f"patch_conv call {i} ({wn}, x {tuple(r['x'].shape)}, k {k} stride {st})"
        assert (k, st, p) == ((3, 2, 1) if i == 0 else S.STAGE_KSP[i - 1])
        D, Cx = r["w"].shape[0], r["x"].shape[-1]
        real = cin if i == 0 else Cx             # (the downsampler's rows and weight are zero-padded from cin to cin_pad channels)
        w4 = r["w"].view(D, Cx, k, k)
        if i == 0:
            assert Cx == m.cin_pad and float(r["x"][..., cin:].float().abs().sum()) == 0.0 and float(w4[:, cin:].abs().sum()) == 0.0
        assert torch.equal(w4[:, :real], params[wn].detach().view(D, real, k, k)) and torch.equal(r["b"], params[bn].detach()), what
        y, dw, db = _node_against_float64(what, lambda a, w, b: S.patch_conv(a, w, b, k, st, p),
                                          lambda a, w, b: N.patch_conv_ref(a, w, b, k, st, p), r["x"], r["w"], r["b"], r["dy"])
        assert torch.equal(y, r["y"]), what
        dw = dw.view(D, Cx, k, k)[:, :real].reshape(got[wn].shape)
        assert T.rel(got[wn], dw) <= PARAM_BAR and T.rel(got[bn], db) <= PARAM_BAR, f"{what}: dw {T.rel(got[wn], dw):.2e} db {T.rel(got[bn], db):.2e}"
    for i, (r, (wn, bn)) in enumerate(zip(rec.linears, lins)):
        what = f"linear call {i} ({wn}, x {tuple(r['x'].shape)} -> {r['w'].shape[0]})"
        assert r["res"] is None and (r["b"] is None) == (bn is None), what
        y, dw, db = _node_against_float64(what, G.linear, N.linear_ref, r["x"], r["w"], r["b"], r["dy"])
        assert torch.equal(y, r["y"]), what
        gw = got[wn]
        if wn == "to_segmentation.0.weight":
            gw = gw.view(dd, 4 * dd)[:, (i // 2) * dd: (i // 2 + 1) * dd]
        elif wn == "to_segmentation.1.weight":      # the head padded to 8 channels: zero rows, cropped after the up-sampling
            assert r["w"].shape[0] == (O + 7) // 8 * 8 and float(r["w"][O:].abs().sum()) == 0.0 and float(r["b"][O:].abs().sum()) == 0.0
            dw, db = dw[:O], db[:O]
        gw = gw.reshape(dw.shape)
        assert T.rel(gw, dw) <= PARAM_BAR, f"{what}: dw {T.rel(gw, dw):.2e}"
        if bn is not None:
            assert T.rel(got[bn], db) <= PARAM_BAR, f"{what}: db {T.rel(got[bn], db):.2e}"
    r = rec.up_sums[0]
    zl = [z.clone().requires_grad_(True) for z in r["z"]]
    y = S.up_sum(*zl)
    assert torch.equal(y, r["y"])
    y.backward(r["dy"])
    z64 = [z.double().requires_grad_(True) for z in r["z"]]
    yr = N.up_sum_ref(*z64)
    gz = torch.autograd.grad(yr, z64, r["dy"].double())
    T.close_bf16(y, yr, "up_sum: y")
    for lv in range(4):
        T.close_bf16(zl[lv].grad, gz[lv], f"up_sum: dz{lv}")
    r = rec.upsamples[0]
    assert r["skip"] is None and r["scale"] == 8 and r["x"].shape[-1] == (O + 7) // 8 * 8
    assert float(r["dy"][..., O:].float().abs().sum()) == 0.0          # the crop hands nothing to the padding channels
    xl = r["x"].clone().requires_grad_(True)
    y = G.upsample_add(xl, None, 8)
    assert torch.equal(y, r["y"])
    y.backward(r["dy"])
    x64 = r["x"].double().requires_grad_(True)
    yr = N.upsample8_ref(x64)
    T.close_bf16(y, yr, "head up-sampling: y")
    T.close_bf16(xl.grad, torch.autograd.grad(yr, x64, r["dy"].double())[0], "head up-sampling: dx")


def test_decoder_weight_slices(cfg):
    """stage i's second linear takes columns [i dd, (i + 1) dd) of to_segmentation.0.weight -- the recorded operand IS that slice --, the
    bias is added once (stage 0), and what up_sum returns is the network's own decoder in float64: Conv2d(4 dd, dd, 1) of the
    concatenated, nearest-up-sampled to_fused outputs (the recorded ones), 2-norm 3e-3"""
    m, rec = cfg["m"], cfg["rec"]
    seg0 = m.to_segmentation[0]
    dd = seg0.out_channels
    w0 = seg0.weight.detach().view(dd, 4 * dd)
    for i in range(4):
        r = rec.linears[2 * i + 1]
        assert torch.equal(r["w"], w0[:, i * dd: (i + 1) * dd]), f"decoder stage {i}: weight slice"
        assert (torch.equal(r["b"], seg0.bias.detach()) if i == 0 else r["b"] is None), f"decoder stage {i}: bias"
        assert torch.equal(r["x"], rec.linears[2 * i]["y"])
    fused = [rec.linears[2 * i]["y"].double() for i in range(4)]
    ref = N.decoder_cat_ref(fused, N._gemm_w(seg0.weight), seg0.bias.detach().double())
    got = rec.up_sums[0]["y"]
    assert got.shape == ref.shape and T.rel(got, ref) <= 3e-3, f"decoder: {T.rel(got, ref):.2e}"


def test_chain_is_exact(cfg):
    """_forward_native's graph on the recorded tensors, bit for bit: rows -> downsampler -> (embedding -> blocks) x 4 -> decoder pairs
    -> up_sum -> head -> up-sampling -> crop -> the returned tensor; every block starts with its LayerNorm on the block's input"""
    m, rec, L = cfg["m"], cfg["rec"], cfg["layers"]
    cin, O = m.in_channels, m.out_channels
    pc, lin = rec.patch_convs, rec.linears
    assert torch.equal(pc[0]["x"][..., :cin], cfg["x"])
    assert torch.equal(pc[1]["x"], pc[0]["y"])
    for s in range(4):
        blocks = rec.blocks[2 * L * s: 2 * L * (s + 1)]
        assert [b["kind"] for b in blocks] == ["attn", "ff"] * L
        feed = pc[s + 1]["y"]
        for j, b in enumerate(blocks):
            assert torch.equal(b["x"], feed), f"stage {s} block {j}"
            assert torch.equal(rec.norms[2 * L * s + j]["x"], b["x"]), f"stage {s} block {j}: LayerNorm input"
            feed = b["y"]
        if s < 3:
            assert torch.equal(pc[s + 2]["x"], feed), f"stage {s} -> embedding {s + 1}"
        assert torch.equal(lin[2 * s]["x"], feed), f"stage {s} -> decoder"
        assert torch.equal(lin[2 * s + 1]["x"], lin[2 * s]["y"])
        assert torch.equal(rec.up_sums[0]["z"][s], lin[2 * s + 1]["y"])
    assert torch.equal(lin[8]["x"], rec.up_sums[0]["y"])
    assert torch.equal(rec.upsamples[0]["x"], lin[8]["y"])
    assert torch.equal(cfg["y"], rec.upsamples[0]["y"][..., :O])


# ------------------------------------------------------------------------------------------------ the f32 flavour
@pytest.mark.parametrize("name", C.NAMES)
def test_f32_flavour_against_restatement(gpu_device, name):
    dev = gpu_device
    m = C.make_model(name, "f32", dev)
    ref = R.reference_from(m).to(dev)
    x, dy = C.make_inputs(name, dev)
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    y.backward(dy)
    xd = x.double().requires_grad_(True)
    yr = R.ref_forward_nhwc(ref, xd)
    yr.backward(dy.double())
    assert y.shape == yr.shape and T.rel(y, yr) <= FP32_BAR, T.rel(y, yr)
    assert T.rel(xg.grad, xd.grad) <= FP32_BAR, T.rel(xg.grad, xd.grad)
    pr = dict(ref.named_parameters())
    for n, p in m.named_parameters():
        assert T.rel(p.grad, pr[n].grad) <= FP32_BAR, (n, T.rel(p.grad, pr[n].grad))


# ------------------------------------------------------------------------------------------------ once, on `narrow`
def test_narrow_sink_route_and_bit_identical_rerun(gpu_device):
    dev = gpu_device
    m = C.make_model("narrow", "bf16", dev)
    x, dy = _inputs("narrow", dev)

    def step():
        m.zero_grad(set_to_none=True)
        y = m(x)
        y.float().backward(dy)
        torch.cuda.synchronize()
        return y.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}

    y1, g1 = step()
    y2, g2 = step()
    assert torch.equal(y1, y2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    T.check_sink_route(m, x, dy, dev)


# ------------------------------------------------------------------------------------------------ refusals
def test_more_than_256_keys_is_refused_on_the_bf16_route_only(gpu_device):
    from py4cast_amd import _lib as L
    from py4cast_amd.segformer import SegformerMI355X, SegformerSettings

    dev = gpu_device
    bf16 = SegformerSettings(reduction_ratio=(1, 1, 1, 1), compute_dtype="bf16", activation_dtype="bf16")
    with pytest.raises(ValueError, match="384"):
        SegformerMI355X(8, 8, (128, 192), bf16)
    m = SegformerMI355X(8, 8, None, bf16).to(dev)
    with pytest.raises(L.P4CError, match="384"):
        m(torch.randn(1, 128, 192, 8, device=dev).to(torch.bfloat16))
    f32 = SegformerSettings(reduction_ratio=(1, 1, 1, 1))
    y = SegformerMI355X(8, 8, (128, 192), f32).to(dev)(torch.randn(1, 128, 192, 8, device=dev))
    assert y.shape == (1, 128, 192, 8) and bool(torch.isfinite(y).all())
