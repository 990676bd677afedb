"""The float64 node references of tests/deeplabv3_nodes.py, composed into the whole DeepLabV3Plus by hand (forward, then the backward node
by node in reverse, each node's decisions -- ReLU masks, the stem's max-pool routing -- taken from this composition's own forward, the
gradients of tensors with several consumers summed as autograd sums them: layer1's output feeds layer2.0's two convolutions and
decoder.block1, layer4's the 1x1 branch, the three-rate depthwise node and the pooling branch), against the autograd of the float64
restatement (tests/deeplabv3plus_reference.py): the references the GPU node tests trust must BE the network, to rounding.  resnet18 and
resnet34, training and eval, the ASPP projection's Dropout at p = 0 and at p = 0.5 with a fixed draw.  Then the new references one by
one against autograd, and the recorder's schedule."""
import copy
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deeplabv3_nodes as N  # noqa: E402
import deeplabv3plus_nodes as M  # noqa: E402
from deeplabv3plus_reference import RATES, SKIP, DeepLabV3PlusReference  # noqa: E402
from test_deeplabv3_nodes_cpu import _randomise, rel  # noqa: E402


def compose(ref, x, dy, mask=None):
    """y, dx, {parameter name: gradient} and {batch-norm name: its node result} of `ref` (float64; its train / eval mode) at x
    (B, H, W, Cin) for the output gradient dy, from the node references alone.  mask (B H/16 W/16, dc) in {0, 1}: the Dropout draw."""
    c = N.Composer(ref)
    put, bna, run = c.put, c.bna, c.running
    cn = lambda *a, **k: N.conv_node(*a, round_weight=False, **k)     # noqa: E731
    e, dec = ref.encoder, ref.decoder
    aspp = dec.aspp[0]
    # ---- forward
    c1 = cn(x, e.conv1.weight, stride=2, pad=3)
    stem = N.stem_node(c1, e.bn1.weight, e.bn1.bias, e.bn1.eps, running=run(e.bn1))
    c.norms["encoder.bn1"] = stem
    arg = N.pool_arg(N.bn_act(c1, e.bn1.weight, e.bn1.bias, e.bn1.eps, running=run(e.bn1)).out)
    blocks, feats = c.blocks_forward(e, ref.geom, stem.pool)
    skip, hx = feats[0], feats[3]
    c0 = cn(hx, aspp.convs[0][0].weight)
    b0 = bna(c0, aspp.convs[0][1])
    dws = [aspp.convs[k][0][0].weight for k in (1, 2, 3)]
    dw3 = N.dw_node(hx, dws, RATES)
    pw = [cn(dw3.ys[k - 1], aspp.convs[k][0][1].weight) for k in (1, 2, 3)]
    bk = [bna(pw[k - 1], aspp.convs[k][1]) for k in (1, 2, 3)]
    br = [b0.out] + [b.out for b in bk]
    pb = aspp.convs[4]
    asp = N.aspp_node(hx, br, pb[1].weight, pb[2].weight, pb[2].bias, pb[2].eps, running=run(pb[2]))
    c.norms["decoder.aspp.0.convs.4.2"] = asp
    pc, pbn = aspp.project[0], aspp.project[1]
    yp = cn(asp.buf, pc.weight)
    drop = dict(mul=mask, factor=1.0 / (1.0 - ref.dropout)) if (mask is not None and c.train) else {}
    bp = bna(yp, pbn, **drop)
    sa, sb = dec.aspp[1], dec.block2[0]
    dwa = N.dw_node(bp.out, [sa[0].weight], (1,))
    pa = cn(dwa.ys[0], sa[1].weight)
    ba = bna(pa, dec.aspp[2])
    s1 = cn(skip, dec.block1[0].weight)
    bs = bna(s1, dec.block1[1])
    ld = ba.out.shape[-1] + SKIP
    cat = N.upcat_node(ba.out, bs.out, 4, ld)
    dwb = N.dw_node(cat, [sb[0].weight], (1,))
    p2 = cn(dwb.ys[0], sb[1].weight)
    b2 = bna(p2, dec.block2[1])
    head = ref.segmentation_head[0]
    z = cn(b2.out, head.weight, head.bias)
    y = N.upsample_node(z, 4)
    # ---- backward, node by node in reverse
    _, dz = N.upsample_node(z, 4, dout=dy)
    _, d, dw, db = cn(b2.out, head.weight, head.bias, dy=dz)
    put(head.weight, dw)
    put(head.bias, db)

    def norm_back(yy, bn, fwd, dout, **kw):
        b = bna(yy, bn, mask=fwd.mask, dout=dout, **kw)
        put(bn.weight, b.dgamma)
        put(bn.bias, b.dbeta)
        return b.dy

    def conv_back(xx, conv, dyy):
        _, dxx, dww, _ = cn(xx, conv.weight, dy=dyy)
        put(conv.weight, dww)
        return dxx

    d = conv_back(dwb.ys[0], sb[1], norm_back(p2, dec.block2[1], b2, d))
    r = N.dw_node(cat, [sb[0].weight], (1,), dys=[d])
    put(sb[0].weight, r.dws[0])
    _, da, dsk = N.upcat_node(ba.out, bs.out, 4, ld, dout=r.dx)
    dskip = conv_back(skip, dec.block1[0], norm_back(s1, dec.block1[1], bs, dsk))
    d = conv_back(dwa.ys[0], sa[1], norm_back(pa, dec.aspp[2], ba, da))
    r = N.dw_node(bp.out, [sa[0].weight], (1,), dys=[d])
    put(sa[0].weight, r.dws[0])
    dbuf = conv_back(asp.buf, pc, norm_back(yp, pbn, bp, r.dx, **drop))
    a = N.aspp_node(hx, br, pb[1].weight, pb[2].weight, pb[2].bias, pb[2].eps, running=run(pb[2]), pooled_stored=asp.pooled, dbuf=dbuf)
    put(pb[1].weight, a.dw)
    put(pb[2].weight, a.dgamma)
    put(pb[2].bias, a.dbeta)
    dh = a.dx + conv_back(hx, aspp.convs[0][0], norm_back(c0, aspp.convs[0][1], b0, a.dbranches[0]))
    dys = [conv_back(dw3.ys[k - 1], aspp.convs[k][0][1], norm_back(pw[k - 1], aspp.convs[k][1], bk[k - 1], a.dbranches[k])) for k in (1, 2, 3)]
    r = N.dw_node(hx, dws, RATES, dys=dys)           # ONE node: dx summed over the three rates, three weight gradients
    for w, g in zip(dws, r.dws):
        put(w, g)
    dh = dh + r.dx                                   # layer4's output: the 1x1 branch, the depthwise node, the pooling branch
    dh = c.blocks_backward(blocks, dh, {0: dskip})   # layer1's output: layer2.0's two convolutions and decoder.block1
    t = N.stem_node(c1, e.bn1.weight, e.bn1.bias, e.bn1.eps, running=run(e.bn1), arg=arg, pool_stored=stem.pool, dpool=dh)
    put(e.bn1.weight, t.dgamma)
    put(e.bn1.bias, t.dbeta)
    _, dx, dw, _ = cn(x, e.conv1.weight, stride=2, pad=3, dy=t.dy)
    put(e.conv1.weight, dw)
    return y, dx, c.grads, c.norms


@pytest.mark.parametrize("name,train,p", [("resnet18", True, 0.0), ("resnet18", True, 0.5), ("resnet18", False, 0.5),
                                          ("resnet34", True, 0.5), ("resnet34", False, 0.0)])
def test_node_references_compose_to_the_restatement(name, train, p):
    torch.manual_seed(0)
    B, H, W, cin, cout, dc = 2, 48, 64, 5, 3, 16
    ref = DeepLabV3PlusReference(cin, cout, name, dc, p).double().train(train)
    _randomise(ref)
    pre = copy.deepcopy(ref)
    x = torch.randn(B, H, W, cin, dtype=torch.float64)
    for b in range(B):                   # (spread samples: the pooling branch's batch norm over B per-sample means)
        x[b] = x[b] * (1.0 + b) + 0.5 * b
    dy = torch.randn(B, H, W, cout, dtype=torch.float64)
    mask = None
    if p > 0:
        mask = (torch.rand(B * (H // 16) * (W // 16), dc) < 1 - p).double()
    y, dx, grads, norms = compose(ref, x, dy, mask)
    xr = x.clone().requires_grad_(True)
    mk = None
    if mask is not None and train:
        mk = mask.view(B, H // 16, W // 16, dc).permute(0, 3, 1, 2)
    yr = ref(xr, dropout_mask=mk)
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


def test_depthwise_reference_matches_autograd():
    """dw_node at R = 3 on a 10 x 6 map: rate 12 is larger than H (the centre tap alone), rate 8 smaller than H but larger than W (the
    column taps alone), rate 2 inside; y_r, dx = the sum over the rates, and every dw_r against the autograd of F.conv2d(groups=C)"""
    torch.manual_seed(2)
    B, H, W, C, rates = 2, 10, 6, 8, (2, 8, 12)
    x = torch.randn(B, H, W, C, dtype=torch.float64)
    ws = [torch.randn(C, 1, 3, 3, dtype=torch.float64) for _ in rates]
    dys = [torch.randn(B, H, W, C, dtype=torch.float64) for _ in rates]
    r = N.dw_node(x, ws, rates, dys=dys)
    xl = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wl = [w.clone().requires_grad_(True) for w in ws]
    ys = [F.conv2d(xl, w, padding=d, dilation=d, groups=C) for w, d in zip(wl, rates)]
    torch.autograd.backward(ys, [g.permute(0, 3, 1, 2) for g in dys])
    for k in range(3):
        assert rel(r.ys[k], ys[k].detach().permute(0, 2, 3, 1)) <= 1e-12
        assert rel(r.dws[k], wl[k].grad) <= 1e-12, k
    assert rel(r.dx, xl.grad.permute(0, 2, 3, 1)) <= 1e-12
    # rate 12 > H, W: only the centre tap sees data; rate 8 > W: no tap to the left or right
    off = r.dws[2].reshape(C, 9)[:, [0, 1, 2, 3, 5, 6, 7, 8]]
    assert bool((off == 0).all()) and bool((r.dws[1].reshape(C, 9)[:, [0, 2, 3, 5, 6, 8]] == 0).all())
    assert bool((r.dws[1].reshape(C, 9)[:, [1, 7]] != 0).all())


def test_upcat_reference_matches_autograd():
    torch.manual_seed(3)
    B, h, w, Ca, Cs, ld, s = 2, 3, 5, 8, 16, 32, 4
    a = torch.randn(B, h, w, Ca, dtype=torch.float64)
    skip = torch.randn(B, s * h, s * w, Cs, dtype=torch.float64)
    dout = torch.randn(B, s * h, s * w, ld, dtype=torch.float64)
    out, da, dskip = N.upcat_node(a, skip, s, ld, dout=dout)
    al, sl = a.permute(0, 3, 1, 2).clone().requires_grad_(True), skip.permute(0, 3, 1, 2).clone().requires_grad_(True)
    want = torch.cat([F.interpolate(al, scale_factor=s, mode="bilinear", align_corners=True), sl,
                      torch.zeros(B, ld - Ca - Cs, s * h, s * w, dtype=torch.float64)], 1)
    want.backward(dout.permute(0, 3, 1, 2))
    assert rel(out, want.detach().permute(0, 2, 3, 1)) <= 1e-12 and bool((out[..., Ca + Cs:] == 0).all())
    assert rel(da, al.grad.permute(0, 2, 3, 1)) <= 1e-12 and torch.equal(dskip, sl.grad.permute(0, 2, 3, 1))


def test_recorder_schedule_counts():
    """the schedule the recorder checks the calls against: resnet18 makes 5 strided (patch) convolutions (conv1, layer2.0 and layer3.0:
    layer4 is dilated, not strided), 24 conv2d_nhwc calls, 27 batch_norm_act calls, 3 depthwise launches (the ASPP's three rates are
    one) and one each of the stem tail, the ASPP assembly, up_cat and the head's up-sampling; resnet34 16 more convolutions and norms"""
    from py4cast_amd.deeplabv3plus import DeepLabV3PlusMI355X, DeepLabV3PlusSettings

    for name, want in (("resnet18", {"patch": 5, "conv": 24, "bn": 27, "stem": 1, "aspp": 1, "dw": 3, "upcat": 1, "up": 1}),
                       ("resnet34", {"patch": 5, "conv": 40, "bn": 43, "stem": 1, "aspp": 1, "dw": 3, "upcat": 1, "up": 1})):
        m = DeepLabV3PlusMI355X(5, 3, None, DeepLabV3PlusSettings(encoder_name=name, decoder_channels=16, encoder_weights=False,
                                                                  compute_dtype="bf16", activation_dtype="bf16"))
        assert M.counts(m) == want, (name, M.counts(m))
        assert [len(mod) for k, _, mod in M.schedule(m) if k == "dw"] == [3, 1, 1]
        assert sorted(M.owned_parameters(m)) == sorted(id(p) for p in m.parameters()), "every parameter belongs to exactly one node"
