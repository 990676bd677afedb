"""
float64-capable restatement of smp's DeepLabV3Plus on a torchvision ResNet encoder, as mfai v5.0.1 wraps it
(config/CLI/model/deeplabv3plus.yaml) -- the oracle of tests/test_deeplabv3plus_*.py: the network written out on torch.nn.functional
(NCHW), with parameters held in plain modules whose state-dict keys are those of py4cast_amd.deeplabv3plus.DeepLabV3PlusMI355X
(torchvision's ResNet keys under ``encoder.``, ``decoder.aspp.0.convs.k``, ``decoder.aspp.0.project``, ``decoder.aspp.{1,2}``,
``decoder.block1``, ``decoder.block2``, ``segmentation_head.0``).  Input / output are features-last (B, H, W, C) like the native model's.

Assumptions (PARITY UNPINNED): BasicBlock ResNet encoder at output stride 16 -- layer strides (1, 2, 2, 1), layer4 dilation 2 with padding
2; separable convolution = depthwise 3x3 (padding = dilation, no bias) then pointwise 1x1 (no bias); ASPP rates (12, 24, 36): 1x1 branch,
three separable branches, the pooling branch broadcast, project 1x1 conv -> BN -> ReLU -> Dropout(p); then a separable 3x3 -> BN -> ReLU;
bilinear x4 (align_corners=True); block1 = 1x1 conv 64 -> 48 -> BN -> ReLU on layer1's map; block2 = separable 3x3 (dc + 48 -> dc) -> BN
-> ReLU on the concatenation; head = 1x1 conv (bias) then bilinear x4 (align_corners=True).

``round_trip``: a callable applied to every stored activation (the convolution outputs -- depthwise and pointwise alike -- the activated
maps, the up-sampled map inside the concatenation and the head's two maps), identity by default -- ``bf16_round_trip`` measures what bf16
storage alone costs this network (tests/test_deeplabv3plus_gpu.py).  The pooling branch stays in full precision (the native route runs it
in fp32) up to its broadcast into the stored concatenation.
"""
import torch
import torch.nn.functional as F
from torch import nn

BLOCKS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}
RATES = (12, 24, 36)
SKIP = 48


def bf16_round_trip(t):
    """t through bf16 storage and back, with the identity as its gradient"""
    return t + (t.detach().to(torch.bfloat16).to(t.dtype) - t.detach())


def _bn(c):
    return nn.BatchNorm2d(c)


def _conv(ci, co, k, bias=False, groups=1):
    return nn.Conv2d(ci, co, k, bias=bias, groups=groups)


def _block(ci, co, down):
    m = nn.Module()
    m.conv1, m.bn1, m.conv2, m.bn2 = _conv(ci, co, 3), _bn(co), _conv(co, co, 3), _bn(co)
    if down:
        m.downsample = nn.Sequential(_conv(ci, co, 1), _bn(co))
    return m


def _separable(ci, co):
    return nn.Sequential(_conv(ci, ci, 3, groups=ci), _conv(ci, co, 1))


class DeepLabV3PlusReference(nn.Module):
    def __init__(self, in_channels, out_channels, encoder_name="resnet18", decoder_channels=256, dropout=0.0, round_trip=None):
        super().__init__()
        dc = decoder_channels
        self.dropout = dropout
        self.round_trip = round_trip
        enc = nn.Module()
        enc.conv1, enc.bn1 = _conv(in_channels, 64, 7), _bn(64)
        ci = 64
        self.geom = [(1, 1), (2, 1), (2, 1), (1, 2)]          # (stride, dilation) per layer after smp's make_dilated(16)
        for i, (n, co) in enumerate(zip(BLOCKS[encoder_name], (64, 128, 256, 512))):
            blocks = []
            for j in range(n):
                blocks.append(_block(ci, co, j == 0 and (ci != co or self.geom[i][0] != 1)))
                ci = co
            setattr(enc, f"layer{i + 1}", nn.Sequential(*blocks))
        self.encoder = enc
        aspp = nn.Module()
        aspp.convs = nn.ModuleList([nn.Sequential(_conv(512, dc, 1), _bn(dc))] + [nn.Sequential(_separable(512, dc), _bn(dc)) for _ in RATES]
                                   + [nn.Sequential(nn.Identity(), _conv(512, dc, 1), _bn(dc))])
        aspp.project = nn.Sequential(_conv(5 * dc, dc, 1), _bn(dc))
        dec = nn.Module()
        dec.aspp = nn.Sequential(aspp, _separable(dc, dc), _bn(dc))
        dec.block1 = nn.Sequential(_conv(64, SKIP, 1), _bn(SKIP))
        dec.block2 = nn.Sequential(_separable(dc + SKIP, dc), _bn(dc))
        self.decoder = dec
        self.segmentation_head = nn.Sequential(_conv(dc, out_channels, 1, bias=True))

    @staticmethod
    def _nrm(bn, x):
        return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.training, bn.momentum, bn.eps)

    def forward_nchw(self, x, dropout_mask=None):
        rt = self.round_trip or (lambda t: t)
        nrm = self._nrm

        def cbr(conv, bn, t, relu=True, **kw):            # stored: the convolution's output and the normalised (activated) map
            y = nrm(bn, rt(F.conv2d(t, conv.weight, **kw)))
            return rt(F.relu(y) if relu else y)

        def sep(s, bn, t, d):                             # stored: the depthwise map, the pointwise map, the activated map
            y = rt(F.conv2d(t, s[0].weight, padding=d, dilation=d, groups=t.shape[1]))
            return cbr(s[1], bn, y)

        e = self.encoder
        h = cbr(e.conv1, e.bn1, x, stride=2, padding=3)
        h = F.max_pool2d(h, 3, stride=2, padding=1)
        skip = None
        for i in range(4):
            s, d = self.geom[i]
            for j, blk in enumerate(getattr(e, f"layer{i + 1}")):
                st = s if j == 0 else 1
                idn = h
                if hasattr(blk, "downsample"):
                    idn = cbr(blk.downsample[0], blk.downsample[1], h, relu=False, stride=st)
                y = cbr(blk.conv1, blk.bn1, h, stride=st, padding=d, dilation=d)
                y = nrm(blk.bn2, rt(F.conv2d(y, blk.conv2.weight, padding=d, dilation=d)))
                h = rt(F.relu(y + idn))
            if i == 0:
                skip = h
        aspp = self.decoder.aspp[0]
        outs = [cbr(aspp.convs[0][0], aspp.convs[0][1], h)]
        for k, r in enumerate(RATES):
            c = aspp.convs[k + 1]
            outs.append(sep(c[0], c[1], h, r))
        pb = aspp.convs[4]
        p = F.relu(nrm(pb[2], F.conv2d(F.adaptive_avg_pool2d(h, 1), pb[1].weight)))
        outs.append(rt(p.expand(-1, -1, h.shape[2], h.shape[3])))
        z = F.relu(nrm(aspp.project[1], rt(F.conv2d(torch.cat(outs, dim=1), aspp.project[0].weight))))
        if dropout_mask is not None:
            z = z * dropout_mask / (1.0 - self.dropout)
        elif self.training and self.dropout > 0:
            z = F.dropout(z, self.dropout)
        z = sep(self.decoder.aspp[1], self.decoder.aspp[2], rt(z), 1)
        up = rt(F.interpolate(z, scale_factor=4, mode="bilinear", align_corners=True))
        s48 = cbr(self.decoder.block1[0], self.decoder.block1[1], skip)
        z = sep(self.decoder.block2[0], self.decoder.block2[1], torch.cat([up, s48], dim=1), 1)
        z = rt(F.conv2d(z, self.segmentation_head[0].weight, self.segmentation_head[0].bias))
        return rt(F.interpolate(z, scale_factor=4, mode="bilinear", align_corners=True))

    def forward(self, x, dropout_mask=None):
        """x (B, H, W, C) -> (B, H, W, out); H and W multiples of 16; dropout_mask (B, dc, H/16, W/16) in {0, 1} or None"""
        if x.shape[1] % 16 or x.shape[2] % 16:
            raise RuntimeError("grid must be a multiple of 16")
        return self.forward_nchw(x.permute(0, 3, 1, 2), dropout_mask).permute(0, 2, 3, 1)
