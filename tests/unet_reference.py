"""
float64 restatement of mfai's UNet (v5.0.1, as the reference's config/CLI/model/unet.yaml selects it) -- the oracle of
tests/test_unet_*.py: plain torch modules, NCHW, torch.cat / nn.MaxPool2d / nn.ConvTranspose2d exactly as the network is written, with
the same state-dict keys as py4cast_amd.unet.UNetMI355X.  Input / output are features-last (B, H, W, C) like the native model's.
"""
from collections import OrderedDict

import torch
from torch import nn


def _block(cin, features, name):
    return nn.Sequential(OrderedDict([
        (name + "conv1", nn.Conv2d(cin, features, 3, padding=1, bias=False)),
        (name + "norm1", nn.BatchNorm2d(features)),
        (name + "relu1", nn.ReLU(inplace=True)),
        (name + "conv2", nn.Conv2d(features, features, 3, padding=1, bias=False)),
        (name + "norm2", nn.BatchNorm2d(features)),
        (name + "relu2", nn.ReLU(inplace=True)),
    ]))


class UNetReference(nn.Module):
    def __init__(self, in_channels, out_channels, init_features=64, autopad=False):
        super().__init__()
        f = init_features
        self.autopad = autopad
        self.encoder1 = _block(in_channels, f, "enc1")
        self.pool1 = nn.MaxPool2d(2, 2)
        self.encoder2 = _block(f, f * 2, "enc2")
        self.pool2 = nn.MaxPool2d(2, 2)
        self.encoder3 = _block(f * 2, f * 4, "enc3")
        self.pool3 = nn.MaxPool2d(2, 2)
        self.encoder4 = _block(f * 4, f * 8, "enc4")
        self.pool4 = nn.MaxPool2d(2, 2)
        self.bottleneck = _block(f * 8, f * 16, "bottleneck")
        self.upconv4 = nn.ConvTranspose2d(f * 16, f * 8, 2, stride=2)
        self.decoder4 = _block(f * 16, f * 8, "dec4")
        self.upconv3 = nn.ConvTranspose2d(f * 8, f * 4, 2, stride=2)
        self.decoder3 = _block(f * 8, f * 4, "dec3")
        self.upconv2 = nn.ConvTranspose2d(f * 4, f * 2, 2, stride=2)
        self.decoder2 = _block(f * 4, f * 2, "dec2")
        self.upconv1 = nn.ConvTranspose2d(f * 2, f, 2, stride=2)
        self.decoder1 = _block(f * 2, f, "dec1")
        self.conv = nn.Conv2d(f, out_channels, 1)

    def forward_nchw(self, x):
        enc1 = self.encoder1(x)
        enc2 = self.encoder2(self.pool1(enc1))
        enc3 = self.encoder3(self.pool2(enc2))
        enc4 = self.encoder4(self.pool3(enc3))
        bottleneck = self.bottleneck(self.pool4(enc4))
        dec4 = self.decoder4(torch.cat((self.upconv4(bottleneck), enc4), dim=1))
        dec3 = self.decoder3(torch.cat((self.upconv3(dec4), enc3), dim=1))
        dec2 = self.decoder2(torch.cat((self.upconv2(dec3), enc2), dim=1))
        dec1 = self.decoder1(torch.cat((self.upconv1(dec2), enc1), dim=1))
        return self.conv(dec1)

    def forward(self, x):
        """x (B, H, W, C) -> (B, H, W, out); autopad: centred zero padding to multiples of 16, then cropped"""
        H, W = x.shape[1], x.shape[2]
        dh, dw = (-H) % 16, (-W) % 16
        top, left = dh // 2, dw // 2
        if dh or dw:
            if not self.autopad:
                raise ValueError("grid must be a multiple of 16")
            x = torch.nn.functional.pad(x, (0, 0, left, dw - left, top, dh - top))
        y = self.forward_nchw(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        return y[:, top: top + H, left: left + W, :]


def padding_for(H, W):
    dh, dw = (-H) % 16, (-W) % 16
    return dh // 2, dh - dh // 2, dw // 2, dw - dw // 2
