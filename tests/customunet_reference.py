"""
float64-capable restatement of smp's Unet on a torchvision ResNet encoder, as mfai v5.0.1's CustomUnet wraps it
(config/CLI/model/customunet.yaml) -- the oracle of tests/test_customunet_*.py: plain torch.nn modules (NCHW), F.interpolate / torch.cat /
nn.MaxPool2d exactly as the network is written, with the state-dict keys of py4cast_amd.customunet.CustomUNetMI355X (torchvision's ResNet
keys under ``encoder.``, ``decoder.blocks.{0..4}.conv{1,2}.{0,1}``, ``segmentation_head.0``).  Input / output are features-last
(B, H, W, C) like the native model's.

Assumptions (PARITY UNPINNED): BasicBlock ResNet, layer strides (1, 2, 2, 2), no dilation; features f1 = relu(bn1(conv1 x)) (stride 2),
f2..f5 = layer1..4 behind the 3x3 / 2 max-pool; decoder widths (256, 128, 64, 32, 16), block = nearest x2 -> cat with the skip (f4, f3,
f2, f1, none) -> twice (3x3 conv without bias, BatchNorm, ReLU); head = 3x3 conv with bias; autopad: centred zero padding to multiples
of 32, then cropped.

``round_trip``: a callable applied to every stored activation (the convolution outputs and the activated maps), identity by default --
``bf16_round_trip`` measures what bf16 storage alone costs this network (tests/test_customunet_gpu.py).
"""
import torch
import torch.nn.functional as F
from torch import nn

BLOCKS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}
DECODER = (256, 128, 64, 32, 16)
SKIPS = (256, 128, 64, 64, 0)


def bf16_round_trip(t):
    """t through bf16 storage and back, with the identity as its gradient"""
    return t + (t.detach().to(torch.bfloat16).to(t.dtype) - t.detach())


class _Block(nn.Module):
    def __init__(self, ci, co, stride):
        super().__init__()
        self.stride = stride
        self.conv1 = nn.Conv2d(ci, co, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(co)
        self.conv2 = nn.Conv2d(co, co, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(co)
        if stride != 1 or ci != co:
            self.downsample = nn.Sequential(nn.Conv2d(ci, co, 1, stride=stride, bias=False), nn.BatchNorm2d(co))

    def forward(self, x, rt):
        idn = x
        if hasattr(self, "downsample"):
            idn = rt(self.downsample[1](rt(self.downsample[0](x))))
        y = rt(F.relu(self.bn1(rt(self.conv1(x)))))
        return rt(F.relu(self.bn2(rt(self.conv2(y))) + idn))


class _DecoderBlock(nn.Module):
    def __init__(self, ci, cs, co):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(ci + cs, co, 3, padding=1, bias=False), nn.BatchNorm2d(co))
        self.conv2 = nn.Sequential(nn.Conv2d(co, co, 3, padding=1, bias=False), nn.BatchNorm2d(co))

    def forward(self, x, skip, rt):
        x = F.interpolate(x, scale_factor=2, mode="nearest")
        if skip is not None:
            x = torch.cat([x, skip], dim=1)
        x = rt(F.relu(self.conv1[1](rt(self.conv1[0](x)))))
        return rt(F.relu(self.conv2[1](rt(self.conv2[0](x)))))


class CustomUNetReference(nn.Module):
    def __init__(self, in_channels, out_channels, encoder_name="resnet18", autopad=False, round_trip=None):
        super().__init__()
        self.autopad = autopad
        self.round_trip = round_trip
        enc = nn.Module()
        enc.conv1, enc.bn1 = nn.Conv2d(in_channels, 64, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64)
        ci = 64
        for i, (n, co, s) in enumerate(zip(BLOCKS[encoder_name], (64, 128, 256, 512), (1, 2, 2, 2))):
            blocks = []
            for j in range(n):
                blocks.append(_Block(ci, co, s if j == 0 else 1))
                ci = co
            setattr(enc, f"layer{i + 1}", nn.ModuleList(blocks))
        self.encoder = enc
        dec = nn.Module()
        dec.blocks = nn.ModuleList([_DecoderBlock(ci_, cs, co) for ci_, cs, co in zip((512,) + DECODER[:-1], SKIPS, DECODER)])
        self.decoder = dec
        self.segmentation_head = nn.Sequential(nn.Conv2d(DECODER[-1], out_channels, 3, padding=1))

    def forward_nchw(self, x):
        rt = self.round_trip or (lambda t: t)
        e = self.encoder
        f1 = rt(F.relu(e.bn1(rt(e.conv1(x)))))
        h = F.max_pool2d(f1, 3, stride=2, padding=1)
        feats = [f1]
        for i in range(4):
            for blk in getattr(e, f"layer{i + 1}"):
                h = blk(h, rt)
            feats.append(h)
        f1, f2, f3, f4, d = feats
        for blk, skip in zip(self.decoder.blocks, (f4, f3, f2, f1, None)):
            d = blk(d, skip, rt)
        return self.segmentation_head(d)

    def forward(self, x):
        """x (B, H, W, C) -> (B, H, W, out); autopad: centred zero padding to multiples of 32, then cropped"""
        H, W = x.shape[1], x.shape[2]
        dh, dw = (-H) % 32, (-W) % 32
        top, left = dh // 2, dw // 2
        if dh or dw:
            if not self.autopad:
                raise ValueError("grid must be a multiple of 32")
            x = F.pad(x, (0, 0, left, dw - left, top, dh - top))
        y = self.forward_nchw(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        return y[:, top: top + H, left: left + W, :]


def padding_for(H, W):
    dh, dw = (-H) % 32, (-W) % 32
    return dh // 2, dh - dh // 2, dw // 2, dw - dw // 2
