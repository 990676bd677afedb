"""The float64 node references of tests/deeplabv3_nodes.py, composed into the whole CustomUNet by hand (forward, then the backward node by
node in reverse, each node's decisions -- ReLU masks, the stem's max-pool routing -- taken from this composition's own forward, the
gradients of tensors with several consumers summed as autograd sums them: f2, f3 and f4 each feed the next layer's conv1, its
downsample and a decoder skip; f1 reaches the stem tail as ``dskip`` beside the pooled map's gradient), against the autograd of the
float64 restatement (tests/customunet_reference.py): the references the GPU node tests trust must BE the network, to rounding.  resnet18
and resnet34, training and eval.  Then the new references one by one against autograd, and the recorder's schedule."""
import copy
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import customunet_nodes as M  # noqa: E402
import deeplabv3_nodes as N  # noqa: E402
from customunet_reference import CustomUNetReference  # noqa: E402
from test_deeplabv3_nodes_cpu import _randomise, rel  # noqa: E402

GEOM = [(1, 1), (2, 1), (2, 1), (2, 1)]      # (stride, dilation) per encoder layer


def compose(ref, x, dy):
    """y, dx, {parameter name: gradient} and {batch-norm name: its node result} of `ref` (float64; its train / eval mode) at x
    (B, H, W, Cin) for the output gradient dy, from the node references alone"""
    c = N.Composer(ref)
    put, bna, run = c.put, c.bna, c.running
    cn = lambda *a, **k: N.conv_node(*a, round_weight=False, **k)     # noqa: E731
    e = ref.encoder
    # ---- forward
    c1 = cn(x, e.conv1.weight, stride=2, pad=3)
    stem = N.stemskip_node(c1, e.bn1.weight, e.bn1.bias, e.bn1.eps, running=run(e.bn1))
    c.norms["encoder.bn1"] = stem
    arg = N.pool_arg(stem.act)
    blocks, feats = c.blocks_forward(e, GEOM, stem.pool)
    f2, f3, f4, d = feats
    dec = []
    for blk, skip in zip(ref.decoder.blocks, (f4, f3, f2, stem.act, None)):
        r = {"blk": blk, "x": d, "skip": skip}
        r["u"] = N.up2cat_node(d, skip)
        r["c1"] = cn(r["u"], blk.conv1[0].weight, pad=1)
        r["b1"] = bna(r["c1"], blk.conv1[1])
        r["c2"] = cn(r["b1"].out, blk.conv2[0].weight, pad=1)
        r["b2"] = bna(r["c2"], blk.conv2[1])
        d = r["b2"].out
        dec.append(r)
    head = ref.segmentation_head[0]
    y = cn(d, head.weight, head.bias, pad=1)
    # ---- backward, node by node in reverse
    _, dd, dw, db = cn(d, head.weight, head.bias, pad=1, dy=dy)
    put(head.weight, dw)
    put(head.bias, db)
    dskips = []
    for r in reversed(dec):
        blk = r["blk"]
        for cv, yy, fwd, xx in ((blk.conv2, r["c2"], r["b2"], r["b1"].out), (blk.conv1, r["c1"], r["b1"], r["u"])):
            b = bna(yy, cv[1], mask=fwd.mask, dout=dd)
            put(cv[1].weight, b.dgamma)
            put(cv[1].bias, b.dbeta)
            _, dd, dw, _ = cn(xx, cv[0].weight, pad=1, dy=b.dy)
            put(cv[0].weight, dw)
        _, dd, ds = N.up2cat_node(r["x"], r["skip"], dout=dd)
        dskips.append(ds)
    _, df1, df2, df3, df4 = dskips                    # (decoder blocks 4 .. 0: none, f1, f2, f3, f4)
    dh = c.blocks_backward(blocks, dd, {2: df4, 1: df3, 0: df2})
    t = N.stemskip_node(c1, e.bn1.weight, e.bn1.bias, e.bn1.eps, running=run(e.bn1), arg=arg, act_stored=stem.act, dpool=dh, dskip=df1)
    put(e.bn1.weight, t.dgamma)
    put(e.bn1.bias, t.dbeta)
    _, dx, dw, _ = cn(x, e.conv1.weight, stride=2, pad=3, dy=t.dy)
    put(e.conv1.weight, dw)
    return y, dx, c.grads, c.norms


@pytest.mark.parametrize("name,train", [("resnet18", True), ("resnet18", False), ("resnet34", True), ("resnet34", False)])
def test_node_references_compose_to_the_restatement(name, train):
    torch.manual_seed(0)
    B, H, W, cin, cout = 2, 64, 96, 5, 3
    ref = CustomUNetReference(cin, cout, name).double().train(train)
    _randomise(ref)
    pre = copy.deepcopy(ref)
    x = torch.randn(B, H, W, cin, dtype=torch.float64)
    for b in range(B):
        x[b] = x[b] * (1.0 + b) + 0.5 * b
    dy = torch.randn(B, H, W, cout, dtype=torch.float64)
    y, dx, grads, norms = compose(ref, x, dy)
    xr = x.clone().requires_grad_(True)
    yr = ref(xr)
    yr.backward(dy)
    assert y.shape == yr.shape == (B, H, W, cout)
    assert rel(y, yr.detach()) <= 1e-10
    assert rel(dx, xr.grad) <= 1e-10
    params = dict(ref.named_parameters())
    assert set(grads) == set(params)
    for n, q in params.items():
        assert grads[n].shape == q.shape, n
        assert rel(grads[n], q.grad) <= 1e-10, (n, rel(grads[n], q.grad))
    if train:
        # the running statistics torch's BatchNorm2d keeps, from each node's batch statistics
        pmods, rmods = dict(pre.named_modules()), dict(ref.named_modules())
        bns = [n for n, m in ref.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]
        assert sorted(norms) == sorted(bns)
        for n in bns:
            rm, rv = N.running_update(pmods[n], norms[n], rmods[n].momentum)
            assert rel(rm, rmods[n].running_mean) <= 1e-12 and rel(rv, rmods[n].running_var) <= 1e-12, n


@pytest.mark.parametrize("Cs,wide", [(16, False), (0, False), (24, True)])
def test_up2cat_reference_matches_autograd(Cs, wide):
    """up2cat_node against the autograd of cat([F.interpolate(nearest x2), skip]); Cs = 0: the up-sampling alone; wide: up2_into's form,
    the skip being the channels a buffer already holds from Cx on"""
    torch.manual_seed(4)
    B, h, w, Cx = 2, 3, 5, 8
    x = torch.randn(B, h, w, Cx, dtype=torch.float64)
    skip = torch.randn(B, 2 * h, 2 * w, Cs, dtype=torch.float64) if Cs else None
    if wide:
        buf = torch.cat([torch.full((B, 2 * h, 2 * w, Cx), float("nan"), dtype=torch.float64), skip], -1)
        skip = buf[..., Cx:]
    dout = torch.randn(B, 2 * h, 2 * w, Cx + Cs, dtype=torch.float64)
    out, dx, dskip = N.up2cat_node(x, skip, dout=dout)
    xl = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    up = F.interpolate(xl, scale_factor=2, mode="nearest")
    sl = None if skip is None else skip.permute(0, 3, 1, 2).clone().requires_grad_(True)
    want = up if sl is None else torch.cat([up, sl], 1)
    want.backward(dout.permute(0, 3, 1, 2))
    assert torch.equal(out, want.detach().permute(0, 2, 3, 1))
    assert rel(dx, xl.grad.permute(0, 2, 3, 1)) <= 1e-12
    assert (dskip is None) if sl is None else torch.equal(dskip, sl.grad.permute(0, 2, 3, 1))


def test_stemskip_reference_matches_relu_skip_max_pool():
    """stemskip_node's arg-routed backward = the autograd of relu -> (skip, max_pool2d(3, 2, 1)) (first maximum wins), odd grid and exact
    ties included"""
    torch.manual_seed(1)
    y = (torch.randint(-8, 9, (2, 11, 13, 8)).double() / 4)
    y[:, :3, :4] = 0.5                          # exact ties
    g, b = torch.rand(8).double() + 0.5, torch.rand(8).double() - 0.5
    t0 = N.stemskip_node(y, g, b, 1e-5)
    arg = N.pool_arg(t0.act)
    assert torch.equal(N.stemskip_node(y, g, b, 1e-5, arg=arg).pool_at_arg, t0.pool)
    dpool = torch.randn(t0.pool.shape, dtype=torch.float64)
    dskip = torch.randn(t0.act.shape, dtype=torch.float64)
    t = N.stemskip_node(y, g, b, 1e-5, arg=arg, act_stored=t0.act, dpool=dpool, dskip=dskip)
    yl = y.clone().requires_grad_(True)
    gl, bl = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    act = torch.relu(F.batch_norm(yl.permute(0, 3, 1, 2), None, None, gl, bl, True, 0.1, 1e-5))
    pool = F.max_pool2d(act, 3, 2, 1)
    assert rel(t0.act, act.detach().permute(0, 2, 3, 1)) <= 1e-12 and rel(t0.pool, pool.detach().permute(0, 2, 3, 1)) <= 1e-12
    torch.autograd.backward([act, pool], [dskip.permute(0, 3, 1, 2), dpool.permute(0, 3, 1, 2)])
    assert rel(t.dy, yl.grad) <= 1e-12 and rel(t.dgamma, gl.grad) <= 1e-12 and rel(t.dbeta, bl.grad) <= 1e-12
    # and without the skip's gradient it is stem_node
    s = N.stem_node(y, g, b, 1e-5, arg=arg, pool_stored=t0.pool, dpool=dpool)
    z = N.stemskip_node(y, g, b, 1e-5, arg=arg, act_stored=t0.act, dpool=dpool, dskip=torch.zeros_like(dskip))
    assert rel(z.dy, s.dy) <= 1e-12


def test_recorder_schedule_counts():
    """the schedule the recorder checks the calls against: resnet18 makes 7 strided (patch) convolutions (conv1 and the first blocks of
    layer2 .. layer4), 24 conv2d_nhwc calls, 29 batch_norm_act calls, the stem tail with its skip, four up2_cat calls and the in-place
    up2_into of decoder block 3; resnet34 16 more convolutions and norms"""
    from py4cast_amd.customunet import CustomUNetMI355X, CustomUNetSettings

    for name, want in (("resnet18", {"patch": 7, "conv": 24, "bn": 29, "stemskip": 1, "up2cat": 4, "up2into": 1}),
                       ("resnet34", {"patch": 7, "conv": 40, "bn": 45, "stemskip": 1, "up2cat": 4, "up2into": 1})):
        m = CustomUNetMI355X(5, 3, None, CustomUNetSettings(encoder_name=name, encoder_weights=False, compute_dtype="bf16", activation_dtype="bf16"))
        assert M.counts(m) == want, (name, M.counts(m))
        assert [n for k, n, _ in M.schedule(m) if k == "up2into"] == ["decoder.blocks.3.up"]
        assert sorted(M.owned_parameters(m)) == sorted(id(p) for p in m.parameters()), "every parameter belongs to exactly one node"
