"""The float64 node references of tests/deeplabv3_nodes.py, composed into the whole DeepLabV3 by hand (forward, then the backward node by
node in reverse, each node's decisions -- ReLU masks, the stem's max-pool routing -- taken from this composition's own forward, the
gradients of tensors with several consumers summed as autograd sums them), against the autograd of the float64 restatement
(tests/deeplabv3_reference.py): the references the GPU node tests trust must BE the network, to rounding.  resnet18 and resnet34,
training and eval, the ASPP projection's Dropout at p = 0 and at p = 0.5 with a fixed draw."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deeplabv3_nodes as N  # noqa: E402
from deeplabv3_reference import DeepLabV3Reference  # noqa: E402

RATES = (12, 24, 36)


def rel(got, ref):
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def compose(ref, x, dy, mask=None):
    """y, dx, {parameter name: gradient} and {batch-norm name: its node result} of `ref` (float64; its train / eval mode) at x
    (B, H, W, Cin) for the output gradient dy, from the node references alone.  mask (B H/8 W/8, dc) in {0, 1}: the Dropout draw."""
    names = {id(p): n for n, p in ref.named_parameters()}
    mods = {id(m): n for n, m in ref.named_modules()}
    grads, norms = {}, {}
    train = ref.training

    def put(p, g):
        n = names[id(p)]
        grads[n] = g if n not in grads else grads[n] + g

    def run(bn):
        return None if train else (bn.running_mean, bn.running_var)

    def bna(y, bn, slope=0.0, **kw):
        r = N.bn_act(y, bn.weight, bn.bias, bn.eps, slope=slope, running=run(bn), **kw)
        norms[mods[id(bn)]] = r
        return r

    e = ref.encoder
    # ---- forward
    c1 = N.conv_node(x, e.conv1.weight, stride=2, pad=3, round_weight=False)
    stem = N.stem_node(c1, e.bn1.weight, e.bn1.bias, e.bn1.eps, running=run(e.bn1))
    norms["encoder.bn1"] = stem
    arg = N.pool_arg(N.bn_act(c1, e.bn1.weight, e.bn1.bias, e.bn1.eps, running=run(e.bn1)).out)
    h = stem.pool
    blocks = []
    for li, (s, d) in enumerate(ref.geom):
        for j, blk in enumerate(getattr(e, f"layer{li + 1}")):
            st = s if j == 0 else 1
            rec = {"x": h, "blk": blk, "st": st, "d": d}
            rec["c1"] = N.conv_node(h, blk.conv1.weight, stride=st, pad=d, dilation=d, round_weight=False)
            if hasattr(blk, "downsample"):
                rec["cd"] = N.conv_node(h, blk.downsample[0].weight, stride=st, round_weight=False)
                rec["bd"] = bna(rec["cd"], blk.downsample[1], slope=1.0)
                idn = rec["bd"].out
            else:
                idn = h
            rec["idn"] = idn
            rec["b1"] = bna(rec["c1"], blk.bn1)
            rec["c2"] = N.conv_node(rec["b1"].out, blk.conv2.weight, pad=d, dilation=d, round_weight=False)
            rec["b2"] = bna(rec["c2"], blk.bn2, res=idn)
            h = rec["b2"].out
            blocks.append(rec)
    aspp = ref.decoder[0]
    hx = h
    br = []
    for k in range(4):
        cv, bn = aspp.convs[k][0], aspp.convs[k][1]
        r = RATES[k - 1] if k else 0
        c = N.conv_node(hx, cv.weight, pad=r, dilation=max(r, 1), round_weight=False)
        br.append((c, bna(c, bn)))
    pb = aspp.convs[4]
    asp = N.aspp_node(hx, [b.out for _, b in br], pb[1].weight, pb[2].weight, pb[2].bias, pb[2].eps, running=run(pb[2]))
    norms["decoder.0.convs.4.2"] = asp
    pc, pbn = aspp.project[0], aspp.project[1]
    yp = N.conv_node(asp.buf, pc.weight, round_weight=False)
    drop = dict(mul=mask, factor=1.0 / (1.0 - ref.dropout)) if (mask is not None and train) else {}
    bp = bna(yp, pbn, **drop)
    yd = N.conv_node(bp.out, ref.decoder[1].weight, pad=1, round_weight=False)
    bdd = bna(yd, ref.decoder[2])
    head = ref.segmentation_head[0]
    z = N.conv_node(bdd.out, head.weight, head.bias, round_weight=False)
    y = N.upsample_node(z, 8)
    # ---- backward, node by node in reverse
    _, dz = N.upsample_node(z, 8, dout=dy)
    _, da, dw, db = N.conv_node(bdd.out, head.weight, head.bias, dy=dz, round_weight=False)
    put(head.weight, dw)
    put(head.bias, db)
    b = bna(yd, ref.decoder[2], mask=bdd.mask, dout=da)
    put(ref.decoder[2].weight, b.dgamma)
    put(ref.decoder[2].bias, b.dbeta)
    _, da, dw, _ = N.conv_node(bp.out, ref.decoder[1].weight, pad=1, dy=b.dy, round_weight=False)
    put(ref.decoder[1].weight, dw)
    b = bna(yp, pbn, mask=bp.mask, dout=da, **drop)
    put(pbn.weight, b.dgamma)
    put(pbn.bias, b.dbeta)
    _, dbuf, dw, _ = N.conv_node(asp.buf, pc.weight, dy=b.dy, round_weight=False)
    put(pc.weight, dw)
    a = N.aspp_node(hx, [b.out for _, b in br], pb[1].weight, pb[2].weight, pb[2].bias, pb[2].eps, running=run(pb[2]),
                    pooled_stored=asp.pooled, dbuf=dbuf)
    put(pb[1].weight, a.dw)
    put(pb[2].weight, a.dgamma)
    put(pb[2].bias, a.dbeta)
    dh = a.dx
    for k in range(4):
        cv, bn = aspp.convs[k][0], aspp.convs[k][1]
        r = RATES[k - 1] if k else 0
        c, bo = br[k]
        bb = bna(c, bn, mask=bo.mask, dout=a.dbranches[k])
        put(bn.weight, bb.dgamma)
        put(bn.bias, bb.dbeta)
        _, dxk, dw, _ = N.conv_node(hx, cv.weight, pad=r, dilation=max(r, 1), dy=bb.dy, round_weight=False)
        put(cv.weight, dw)
        dh = dh + dxk                      # the ASPP input's five consumers
    for rec in reversed(blocks):
        blk, st, d = rec["blk"], rec["st"], rec["d"]
        b2 = bna(rec["c2"], blk.bn2, res=rec["idn"], mask=rec["b2"].mask, dout=dh)
        put(blk.bn2.weight, b2.dgamma)
        put(blk.bn2.bias, b2.dbeta)
        _, db1, dw, _ = N.conv_node(rec["b1"].out, blk.conv2.weight, pad=d, dilation=d, dy=b2.dy, round_weight=False)
        put(blk.conv2.weight, dw)
        b1 = bna(rec["c1"], blk.bn1, mask=rec["b1"].mask, dout=db1)
        put(blk.bn1.weight, b1.dgamma)
        put(blk.bn1.bias, b1.dbeta)
        _, dx1, dw, _ = N.conv_node(rec["x"], blk.conv1.weight, stride=st, pad=d, dilation=d, dy=b1.dy, round_weight=False)
        put(blk.conv1.weight, dw)
        if "cd" in rec:
            bd = bna(rec["cd"], blk.downsample[1], slope=1.0, dout=b2.dres)
            put(blk.downsample[1].weight, bd.dgamma)
            put(blk.downsample[1].bias, bd.dbeta)
            _, dxd, dw, _ = N.conv_node(rec["x"], blk.downsample[0].weight, stride=st, dy=bd.dy, round_weight=False)
            put(blk.downsample[0].weight, dw)
            dh = dx1 + dxd                 # the block input's two consumers
        else:
            dh = dx1 + b2.dres             # the identity edge (conv1's passthrough on the device)
    t = N.stem_node(c1, e.bn1.weight, e.bn1.bias, e.bn1.eps, running=run(e.bn1), arg=arg, pool_stored=stem.pool, dpool=dh)
    put(e.bn1.weight, t.dgamma)
    put(e.bn1.bias, t.dbeta)
    _, dx, dw, _ = N.conv_node(x, e.conv1.weight, stride=2, pad=3, dy=t.dy, round_weight=False)
    put(e.conv1.weight, dw)
    return y, dx, grads, norms


def _randomise(ref):
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
                m.running_mean.uniform_(-0.5, 0.5)
                m.running_var.uniform_(0.5, 2.0)
            elif getattr(m, "bias", None) is not None:
                m.bias.uniform_(-0.3, 0.3)
            if isinstance(m, torch.nn.Conv2d):
                fan = m.weight[0].numel()
                m.weight.normal_(0, (2.0 / fan) ** 0.5)


@pytest.mark.parametrize("name,train,p", [("resnet18", True, 0.0), ("resnet18", True, 0.5), ("resnet18", False, 0.5),
                                          ("resnet34", True, 0.5), ("resnet34", False, 0.0)])
def test_node_references_compose_to_the_restatement(name, train, p):
    torch.manual_seed(0)
    B, H, W, cin, cout, dc = 2, 48, 64, 5, 3, 16
    ref = DeepLabV3Reference(cin, cout, name, dc, p).double().train(train)
    _randomise(ref)
    pre = copy.deepcopy(ref)
    x = torch.randn(B, H, W, cin, dtype=torch.float64)
    for b in range(B):                   # (spread samples: the pooling branch's batch norm over B per-sample means)
        x[b] = x[b] * (1.0 + b) + 0.5 * b
    dy = torch.randn(B, H, W, cout, dtype=torch.float64)
    mask = None
    if p > 0:
        mask = (torch.rand(B * (H // 8) * (W // 8), dc) < 1 - p).double()
    y, dx, grads, norms = compose(ref, x, dy, mask)
    xr = x.clone().requires_grad_(True)
    mk = None
    if mask is not None and train:
        mk = mask.view(B, H // 8, W // 8, dc).permute(0, 3, 1, 2)
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


def test_stem_routing_reference_matches_max_pool():
    """stem_node's arg-routed backward = the autograd of relu -> max_pool2d(3, 2, 1) (first maximum wins), odd grid and ties included"""
    torch.manual_seed(1)
    y = (torch.randint(-8, 9, (2, 11, 14, 8)).double() / 4)
    y[:, :3, :4] = 0.5                          # exact ties
    g, b = torch.rand(8).double() + 0.5, torch.rand(8).double() - 0.5
    a = N.bn_act(y, g, b, 1e-5).out
    arg = N.pool_arg(a)
    t0 = N.stem_node(y, g, b, 1e-5, arg=arg)
    assert torch.equal(t0.pool, t0.pool_at_arg)
    dpool = torch.randn(t0.pool.shape, dtype=torch.float64)
    t = N.stem_node(y, g, b, 1e-5, arg=arg, pool_stored=t0.pool, dpool=dpool)
    yl = y.clone().requires_grad_(True)
    gl, bl = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    z = torch.nn.functional.batch_norm(yl.permute(0, 3, 1, 2), None, None, gl, bl, True, 0.1, 1e-5)
    pool = torch.nn.functional.max_pool2d(torch.relu(z), 3, 2, 1)
    pool.backward(dpool.permute(0, 3, 1, 2))
    assert rel(t.dy, yl.grad) <= 1e-12 and rel(t.dgamma, gl.grad) <= 1e-12 and rel(t.dbeta, bl.grad) <= 1e-12


def test_recorder_schedule_counts():
    """the schedule the recorder checks the calls against: resnet18 makes 3 strided (patch) convolutions, 24 conv2d_nhwc calls, 25
    batch_norm_act calls and one each of the stem tail, the ASPP assembly and the up-sampling; resnet34 29 more convolutions and norms"""
    from py4cast_amd.deeplabv3 import DeepLabV3MI355X, DeepLabV3Settings

    for name, want in (("resnet18", {"patch": 3, "conv": 24, "bn": 25, "stem": 1, "aspp": 1, "up": 1}),
                       ("resnet34", {"patch": 3, "conv": 40, "bn": 41, "stem": 1, "aspp": 1, "up": 1})):
        m = DeepLabV3MI355X(5, 3, None, DeepLabV3Settings(encoder_name=name, decoder_channels=16, encoder_weights=False,
                                                          compute_dtype="bf16", activation_dtype="bf16"))
        assert N.counts(m) == want, (name, N.counts(m))
        owned = [id(p) for _, _, mod in N.schedule(m) if not isinstance(mod, torch.nn.UpsamplingBilinear2d) for p in mod.parameters()]
        assert sorted(owned) == sorted(id(p) for p in m.parameters()), "every parameter belongs to exactly one node"
