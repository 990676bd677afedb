"""
float64 restatement of smp's DeepLabV3 as mfai v5.0.1 builds it (config/CLI/model/deeplabv3.yaml) -- the oracle of tests/test_deeplabv3_*.py:
the network written out on torch.nn.functional (NCHW), with parameters held in plain modules whose state-dict keys are those of
py4cast_amd.deeplabv3.DeepLabV3MI355X (torchvision's ResNet keys under ``encoder.``, ``decoder.0.convs.k``, ``decoder.0.project``,
``segmentation_head.0``).  Input / output are features-last (B, H, W, C) like the native model's.

Assumptions (PARITY UNPINNED): BasicBlock ResNet encoder with output stride 8 -- layer3 dilation 2, layer4 dilation 4, both stride 1,
padding = dilation for the 3x3 convolutions; ASPP rates (12, 24, 36) with the pooling branch broadcast; project 1x1 conv -> BN -> ReLU
-> Dropout(p); head 1x1 conv (bias) then bilinear x8 with align_corners=True.
"""
import torch
import torch.nn.functional as F
from torch import nn

BLOCKS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}


def _bn(c):
    return nn.BatchNorm2d(c)


def _conv(ci, co, k, bias=False):
    return nn.Conv2d(ci, co, k, bias=bias)


def _block(ci, co, down):
    m = nn.Module()
    m.conv1, m.bn1, m.conv2, m.bn2 = _conv(ci, co, 3), _bn(co), _conv(co, co, 3), _bn(co)
    if down:
        m.downsample = nn.Sequential(_conv(ci, co, 1), _bn(co))
    return m


class DeepLabV3Reference(nn.Module):
    def __init__(self, in_channels, out_channels, encoder_name="resnet18", decoder_channels=256, dropout=0.0):
        super().__init__()
        dc = decoder_channels
        self.dropout = dropout
        enc = nn.Module()
        enc.conv1, enc.bn1 = _conv(in_channels, 64, 7), _bn(64)
        ci = 64
        # (stride, dilation) per layer after smp's make_dilated(8)
        self.geom = [(1, 1), (2, 1), (1, 2), (1, 4)]
        for i, (n, co) in enumerate(zip(BLOCKS[encoder_name], (64, 128, 256, 512))):
            blocks = []
            for j in range(n):
                blocks.append(_block(ci, co, j == 0 and (ci != co or self.geom[i][0] != 1)))
                ci = co
            setattr(enc, f"layer{i + 1}", nn.Sequential(*blocks))
        self.encoder = enc
        aspp = nn.Module()
        aspp.convs = nn.ModuleList([nn.Sequential(_conv(512, dc, 1), _bn(dc))] + [nn.Sequential(_conv(512, dc, 3), _bn(dc)) for _ in range(3)]
                                   + [nn.Sequential(nn.Identity(), _conv(512, dc, 1), _bn(dc))])
        aspp.project = nn.Sequential(_conv(5 * dc, dc, 1), _bn(dc))
        self.decoder = nn.Sequential(aspp, _conv(dc, dc, 3), _bn(dc))
        self.segmentation_head = nn.Sequential(_conv(dc, out_channels, 1, bias=True))

    @staticmethod
    def _nrm(bn, x):
        return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.training, bn.momentum, bn.eps)

    def forward_nchw(self, x, dropout_mask=None):
        e = self.encoder
        h = F.relu(self._nrm(e.bn1, F.conv2d(x, e.conv1.weight, stride=2, padding=3)))
        h = F.max_pool2d(h, 3, stride=2, padding=1)
        for i in range(4):
            s, d = self.geom[i]
            for j, blk in enumerate(getattr(e, f"layer{i + 1}")):
                st = s if j == 0 else 1
                idn = h
                if hasattr(blk, "downsample"):
                    idn = self._nrm(blk.downsample[1], F.conv2d(h, blk.downsample[0].weight, stride=st))
                y = F.relu(self._nrm(blk.bn1, F.conv2d(h, blk.conv1.weight, stride=st, padding=d, dilation=d)))
                y = self._nrm(blk.bn2, F.conv2d(y, blk.conv2.weight, padding=d, dilation=d))
                h = F.relu(y + idn)
        aspp = self.decoder[0]
        outs = [F.relu(self._nrm(aspp.convs[0][1], F.conv2d(h, aspp.convs[0][0].weight)))]
        for k, r in enumerate((12, 24, 36)):
            c = aspp.convs[k + 1]
            outs.append(F.relu(self._nrm(c[1], F.conv2d(h, c[0].weight, padding=r, dilation=r))))
        pb = aspp.convs[4]
        p = F.relu(self._nrm(pb[2], F.conv2d(F.adaptive_avg_pool2d(h, 1), pb[1].weight)))
        outs.append(p.expand(-1, -1, h.shape[2], h.shape[3]))
        z = F.relu(self._nrm(aspp.project[1], F.conv2d(torch.cat(outs, dim=1), aspp.project[0].weight)))
        if dropout_mask is not None:
            z = z * dropout_mask / (1.0 - self.dropout)
        elif self.training and self.dropout > 0:
            z = F.dropout(z, self.dropout)
        z = F.relu(self._nrm(self.decoder[2], F.conv2d(z, self.decoder[1].weight, padding=1)))
        z = F.conv2d(z, self.segmentation_head[0].weight, self.segmentation_head[0].bias)
        return F.interpolate(z, scale_factor=8, mode="bilinear", align_corners=True)

    def forward(self, x, dropout_mask=None):
        """x (B, H, W, C) -> (B, H, W, out); H and W multiples of 8; dropout_mask (B, dc, H/8, W/8) in {0, 1} or None"""
        if x.shape[1] % 8 or x.shape[2] % 8:
            raise RuntimeError("grid must be a multiple of 8")
        return self.forward_nchw(x.permute(0, 3, 1, 2), dropout_mask).permute(0, 2, 3, 1)
