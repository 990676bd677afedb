"""
CustomUNet on MI355X -- the model behind ``model_name: CustomUNet`` (the reference's config/CLI/model/customunet.yaml).  The reference takes
the class from mfai v5.0.1 (``CustomUnet``), which wraps segmentation_models_pytorch's ``Unet`` on a torchvision ResNet; neither is
installed here: PARITY UNPINNED.  The network is smp's Unet as its public documentation and torchvision's ResNet describe it, restated in
tests/customunet_reference.py (float64) and checked against that.

Assumptions (the architecture as written here):
* encoder (state-dict keys ``encoder.*`` = torchvision's ResNet keys without ``fc``): conv1 7x7 / 2 / padding 3 (no bias) -> bn1 -> ReLU
  = f1 (64 channels, stride 2) -> max-pool 3x3 / 2 / padding 1 -> layer1 = f2 (64, stride 4) -> layer2 = f3 (128, stride 8) -> layer3 = f4
  (256, stride 16) -> layer4 = f5 (512, stride 32); BasicBlocks (resnet18 [2, 2, 2, 2], resnet34 [3, 4, 6, 3]), layer strides (1, 2, 2, 2),
  no dilation: the undilated form of deeplabv3.ResNetEncoder;
* decoder (keys ``decoder.blocks.{0..4}.conv{1,2}.{0,1}.*``): centre = identity, widths (256, 128, 64, 32, 16); block i:
  x = nearest_x2(x); x = cat([x, skip], channels) when a skip exists; then twice (3x3 conv, padding 1, no bias -> BatchNorm -> ReLU).
  Skips f4, f3, f2, f1, none: input widths 512 + 256, 256 + 128, 128 + 64, 64 + 64, 32;
* ``segmentation_head.0`` = 3x3 conv 16 -> out_channels, padding 1, with bias; no activation;
* ``autopad_enabled``: grids that are not a multiple of 32 are zero-padded (centred, the extra row / column at the end, as mfai's
  AutoPaddingModel does) and the output cropped; off, such a grid raises;
* initialisation: encoder convs kaiming-normal (fan_out, relu), decoder convs kaiming-uniform (fan_in, relu), head xavier-uniform with
  zero bias, BN weight 1 / bias 0.  ``encoder_weights: True`` never downloads (deeplabv3.load_encoder_weights).

What runs where, bf16 (``compute_dtype`` / ``activation_dtype`` "bf16"), features-last (B, H, W, C) throughout:
* stride-1 3x3 and 1x1 convolutions: ``ops_gemm.conv2d_nhwc`` with the batch-norm statistics from the GEMM epilogue; BN (+ residual) +
  ReLU: ``ops_gemm.batch_norm_act``; the residual block is DeepLabV3MI355X._block (the residual through ``passthrough``);
* the strided convolutions (conv1 7x7 / 2; conv1 3x3 / 2 and downsample 1x1 / 2 of layer2.0, layer3.0, layer4.0): patch gather + one GEMM
  (``ops_patch._PatchConv``);
* the stem tail: bn1 + ReLU, f1 written straight into decoder block 3's concatenation buffer, and the 3x3 / 2 max-pool, in one pass each
  way (csrc/customunet.hip: ``p4c_customunet_stem_fwd / _bwd``);
* every decoder block's nearest x2 up-sampling + concatenation: one pass each way (``p4c_up2_cat_fwd / _bwd``); block 3's pass writes only
  its own channels beside f1.  No F.interpolate, torch.cat, max_pool2d, library convolution or GEMM in a training step.
fp32 (the parity flavour): the same network on library operations (NCHW inside); it runs on the CPU too.
"""

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from . import ops_gemm as G
from .base import ModelType
from .conv_model import ConvModelMI355X, cast_out, crop_channels, pad_head, pad_rows
from .deeplabv3 import ENCODER_BLOCKS, DeepLabV3MI355X, ResNetEncoder, load_encoder_weights

try:
    from dataclasses_json import dataclass_json
except Exception:  # pragma: no cover
    def dataclass_json(cls):
        return cls


DECODER_CHANNELS = (256, 128, 64, 32, 16)
SKIP_CHANNELS = (256, 128, 64, 64, 0)       # f4, f3, f2, f1, none


@dataclass_json
@dataclass
class CustomUNetSettings:
    """mfai's CustomUnetSettings fields (config/CLI/model/customunet.yaml) + the MI355X knobs."""

    encoder_name: str = "resnet18"
    encoder_depth: int = 5
    encoder_weights: bool = True
    autopad_enabled: bool = False   # grids that are not a multiple of 32 are zero-padded (centred) and the output cropped
    # MI355X-specific
    compute_dtype: str = "f32"      # "f32" (library operations, the parity flavour) or "bf16" (the native route)
    activation_dtype: Optional[str] = None   # HBM storage of activations: "f32" | "bf16"; None = compute_dtype
    encoder_weights_path: Optional[str] = None   # a torchvision resnet checkpoint (.pth); None: look in torch.hub's checkpoint cache


# ---------------------------------------------------------------- module tree (keys as smp)
def _conv_bn_relu(cin: int, cout: int) -> nn.Sequential:
    return nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))


class DecoderBlock(nn.Module):
    def __init__(self, cin: int, cskip: int, cout: int):
        super().__init__()
        self.conv1 = _conv_bn_relu(cin + cskip, cout)
        self.conv2 = _conv_bn_relu(cout, cout)

    def forward(self, x, skip=None):
        x = F.interpolate(x, scale_factor=2, mode="nearest")
        if skip is not None:
            x = torch.cat([x, skip], dim=1)
        return self.conv2(self.conv1(x))


class UnetDecoder(nn.Module):
    def __init__(self):
        super().__init__()
        cins = (512,) + DECODER_CHANNELS[:-1]
        self.blocks = nn.ModuleList([DecoderBlock(ci, cs, co) for ci, cs, co in zip(cins, SKIP_CHANNELS, DECODER_CHANNELS)])


# ---------------------------------------------------------------- native nodes
def _check_map(x: torch.Tensor, what: str) -> None:
    if x.dtype != torch.bfloat16 or x.dim() != 4 or x.shape[-1] % 8 or not x.shape[-1]:
        raise L.P4CError(f"customunet.{what}: unsupported map {tuple(x.shape)} {x.dtype} (bf16 (B, H, W, C), C a multiple of 8)")


class _Up2Cat(torch.autograd.Function):
    """out (B, 2h, 2w, Cx + Cs) = cat([nearest_x2(x), skip], channels) (skip None: the up-sampling alone); one native pass each way"""

    @staticmethod
    def forward(ctx, x, skip):
        xc = x.contiguous()
        B, h, w, Cx = xc.shape
        sc = None if skip is None else skip.contiguous()
        Cs = 0 if sc is None else sc.shape[-1]
        out = torch.empty(B, 2 * h, 2 * w, Cx + Cs, dtype=xc.dtype, device=xc.device)
        L.call("p4c_up2_cat_fwd", L.ptr(xc), L.ptr(sc), L.ptr(out), Cx + Cs, B, h, w, Cx, Cs, L.stream(xc.device),
               alg_bytes=2 * (xc.numel() + out.numel() + (0 if sc is None else sc.numel())))
        ctx.geom = (B, h, w, Cx, Cs)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, h, w, Cx, Cs = ctx.geom
        dout = dout.contiguous()
        dev = dout.device
        dx = torch.empty(B, h, w, Cx, dtype=dout.dtype, device=dev)
        dskip = torch.empty(B, 2 * h, 2 * w, Cs, dtype=dout.dtype, device=dev) if Cs else None
        L.call("p4c_up2_cat_bwd", L.ptr(dout), Cx + Cs, L.ptr(dx), L.ptr(dskip), B, h, w, Cx, Cs, L.stream(dev),
               alg_bytes=2 * (dout.numel() + dx.numel() + (0 if dskip is None else dskip.numel())))
        return dx, dskip


class _Up2Into(torch.autograd.Function):
    """buf[..., :Cx] = nearest_x2(x) in place (buf (B, 2h, 2w, >= Cx): its other channels hold the skip their producer wrote); returns
    buf.  Backward: dx from the first Cx channels of the incoming gradient; the gradient itself is handed on to buf's producer, which
    reads only its own channel slice of it (the stem tail, ``dskip`` in place) -- no slice copy, no zero fill of the first Cx channels"""

    @staticmethod
    def forward(ctx, x, buf):
        xc = x.contiguous()
        B, h, w, Cx = xc.shape
        L.call("p4c_up2_cat_fwd", L.ptr(xc), None, L.ptr(buf), buf.shape[-1], B, h, w, Cx, buf.shape[-1] - Cx, L.stream(xc.device),
               alg_bytes=2 * 5 * xc.numel())
        ctx.mark_dirty(buf)
        ctx.geom = (B, h, w, Cx, buf.shape[-1])
        return buf

    @staticmethod
    def backward(ctx, dbuf):
        B, h, w, Cx, ld = ctx.geom
        dbuf = dbuf.contiguous()
        dx = torch.empty(B, h, w, Cx, dtype=dbuf.dtype, device=dbuf.device)
        L.call("p4c_up2_cat_bwd", L.ptr(dbuf), ld, L.ptr(dx), None, B, h, w, Cx, ld - Cx, L.stream(dbuf.device), alg_bytes=2 * 5 * dx.numel())
        return dx, dbuf


def up2_cat(x: torch.Tensor, skip: Optional[torch.Tensor]) -> torch.Tensor:
    """``torch.cat([F.interpolate(x, scale_factor=2, mode="nearest"), skip], channels)`` of features-last bf16 maps x (B, h, w, Cx) and
    skip (B, 2h, 2w, Cs) (None: the up-sampling alone), Cx and Cs multiples of 8"""
    L.require_cuda(x, skip)
    _check_map(x, "up2_cat")
    if skip is not None:
        _check_map(skip, "up2_cat")
        if skip.shape[:3] != (x.shape[0], 2 * x.shape[1], 2 * x.shape[2]):
            raise L.P4CError(f"customunet.up2_cat: skip {tuple(skip.shape)} is not the x2 grid of x {tuple(x.shape)}")
    return _Up2Cat.apply(x, skip)


def up2_into(x: torch.Tensor, buf: torch.Tensor) -> torch.Tensor:
    """``buf[..., :Cx] = F.interpolate(x, scale_factor=2, mode="nearest")`` in place on features-last bf16 maps (x (B, h, w, Cx), buf a
    dense (B, 2h, 2w, >= Cx) buffer); returns buf.  buf's producer must take its gradient from its own channels of the gradient of buf
    (stem_tail_skip does): the first Cx channels of what it receives are the up-sampling's, not zeros."""
    L.require_cuda(x, buf)
    _check_map(x, "up2_into")
    _check_map(buf, "up2_into")
    if buf.shape[:3] != (x.shape[0], 2 * x.shape[1], 2 * x.shape[2]) or buf.shape[-1] < x.shape[-1] or not buf.is_contiguous():
        raise L.P4CError(f"customunet.up2_into: buf {tuple(buf.shape)} is not a dense x2 buffer for x {tuple(x.shape)}")
    return _Up2Into.apply(x, buf)


class _StemTailSkip(torch.autograd.Function):
    """(buf, pool): act = relu(bn(y)) written into buf[..., offset:] (buf (B, H, W, offset + C), its first channels left for up2_into)
    and pool = max_pool2d(act, 3, 2, 1); one native pass each way (csrc/customunet.hip) + the batch norm's finalize / apply"""

    @staticmethod
    def forward(ctx, y, stats, gamma, beta, bn, training, offset):
        yc = y.contiguous()
        B, H, W, C = yc.shape
        dev = yc.device
        st = G.bn_statistics(yc, stats, bn, training)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        buf = torch.empty(B, H, W, offset + C, dtype=yc.dtype, device=dev)
        pool = torch.empty(B, Ho, Wo, C, dtype=yc.dtype, device=dev)
        arg = torch.empty(B, Ho, Wo, C, dtype=torch.uint8, device=dev)
        L.call("p4c_customunet_stem_fwd", L.ptr(yc), L.ptr(st[2]), L.ptr(st[3]), L.ptr(buf[..., offset:]), offset + C, L.ptr(pool), L.ptr(arg),
               B, H, W, C, L.stream(dev), alg_bytes=4 * yc.numel() + 3 * pool.numel())
        ctx.save_for_backward(yc, st, arg)
        ctx.training, ctx.has_affine, ctx.offset = bool(training), gamma is not None, offset
        return buf, pool

    @staticmethod
    def backward(ctx, dbuf, dpool):
        yc, st, arg = ctx.saved_tensors
        B, H, W, C = yc.shape
        dev = yc.device
        dbuf, dpool = dbuf.contiguous(), dpool.contiguous()
        nb = L.lib().p4c_customunet_stem_bwd_blocks(B, H, W, C)
        part = torch.empty(1, nb, 2, C, dtype=torch.float32, device=dev)
        dz = torch.empty_like(yc)
        L.call("p4c_customunet_stem_bwd", L.ptr(yc), L.ptr(dbuf[..., ctx.offset:]), ctx.offset + C, L.ptr(dpool), L.ptr(arg), L.ptr(st[2]),
               L.ptr(st[3]), L.ptr(st[0]), L.ptr(st[1]), L.ptr(dz), L.ptr(part), B, H, W, C, L.stream(dev),
               alg_bytes=6 * yc.numel() + 3 * dpool.numel())
        dy, dg, db = G.bn_tail_backward(yc, dz, part, nb, st, ctx.training, ctx.has_affine)
        return dy, None, dg, db, None, None, None


def stem_tail_skip(y: torch.Tensor, stats, bn: nn.BatchNorm2d, offset: int):
    """(buf (B, H, W, offset + C) with buf[..., offset:] = relu(bn(y)), max_pool2d(relu(bn(y)), 3, stride=2, padding=1)) of a
    features-last bf16 map y (B, H, W, C), C a multiple of 4 up to 1024, offset a multiple of 8; ``stats``: the producer's column sums or
    None.  buf[..., :offset] is uninitialised: up2_into fills it."""
    L.require_cuda(y)
    if y.dtype != torch.bfloat16 or y.dim() != 4 or y.shape[-1] % 4 or y.shape[-1] > 1024 or offset < 0 or offset % 8:
        raise L.P4CError(f"customunet.stem_tail_skip: unsupported map {tuple(y.shape)} {y.dtype} at channel offset {offset}")
    training = bn.training or bn.running_mean is None
    return _StemTailSkip.apply(y, stats if training else None, bn.weight, bn.bias, bn, training, int(offset))


# ---------------------------------------------------------------- the model
class CustomUNetMI355X(ConvModelMI355X):
    """smp's Unet on a ResNet encoder as mfai builds it (module docstring) on the native kernels of this package."""

    settings_kls = CustomUNetSettings
    model_type = ModelType.CONVOLUTIONAL

    def __init__(self, in_channels: int, out_channels: int, input_shape: tuple = None, settings: CustomUNetSettings = CustomUNetSettings(),
                 *args, **kwargs):
        super().__init__(in_channels, out_channels, input_shape, settings)
        s = settings
        if s.encoder_name not in ENCODER_BLOCKS:
            raise ValueError(f"CustomUNetMI355X: encoder_name {s.encoder_name!r} is not served (one of {sorted(ENCODER_BLOCKS)})")
        if s.encoder_depth != 5:
            raise ValueError(f"CustomUNetMI355X: encoder_depth {s.encoder_depth} is not served (5)")
        self._resolve_dtypes(s)
        self.encoder = ResNetEncoder(in_channels, ENCODER_BLOCKS[s.encoder_name], strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1))
        self.decoder = UnetDecoder()
        self.segmentation_head = nn.Sequential(nn.Conv2d(DECODER_CHANNELS[-1], out_channels, 3, padding=1))
        self._init_weights()
        if s.encoder_weights:
            load_encoder_weights(self.encoder, s.encoder_name, in_channels, s.encoder_weights_path, owner="CustomUNetMI355X")
        self.prefers_hip_graph = False     # eager 24.6 ms vs replay 24.7 ms per bench step (profiles/customunet_bf16_bench_*.json)
        self.timed_entry_points = ("p4c_gemm_nt", "p4c_gemm_tn", "p4c_seg_patch_gather", "p4c_seg_patch_scatter", "p4c_customunet_stem_fwd",
                                   "p4c_customunet_stem_bwd", "p4c_up2_cat_fwd", "p4c_up2_cat_bwd", "p4c_inorm_apply")
        self.check_required_attributes()

    _init_weights = DeepLabV3MI355X._init_weights       # encoder / decoder / head / BN exactly as there
    _patch = staticmethod(DeepLabV3MI355X._patch)       # strided convolution: patch gather + GEMM
    _block = DeepLabV3MI355X._block                     # BasicBlock on the native nodes (strided first blocks through _patch)

    def padding_for(self, H: int, W: int):
        """(top, bottom, left, right) zero padding that takes (H, W) to the next multiple of 32 (the encoder's five halvings), centred as
        mfai's AutoPaddingModel does (extra row / column at the end); all zeros when the grid already fits."""
        dh, dw = (-H) % 32, (-W) % 32
        return dh // 2, dh - dh // 2, dw // 2, dw - dw // 2

    # ---------------------------------------------------------------- the bf16 route
    @staticmethod
    def _conv_bn_relu(seq: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
        y, st = G.conv2d_nhwc(x, seq[0].weight, want_stats=True)
        return G.batch_norm_act(y, st, seq[1], slope=0.0)

    def _forward_native(self, x: torch.Tensor) -> torch.Tensor:
        enc, blocks = self.encoder, self.decoder.blocks
        y, st = self._patch(enc.conv1, x)
        buf3, h = stem_tail_skip(y, st, enc.bn1, DECODER_CHANNELS[2])      # f1 beside block 3's up-sampled input
        feats = []
        for layer in (enc.layer1, enc.layer2, enc.layer3, enc.layer4):
            for blk in layer:
                h = self._block(blk, h)
            feats.append(h)
        f2, f3, f4, d = feats
        for i, skip in enumerate((f4, f3, f2)):
            d = self._conv_bn_relu(blocks[i].conv2, self._conv_bn_relu(blocks[i].conv1, up2_cat(d, skip)))
        d = self._conv_bn_relu(blocks[3].conv2, self._conv_bn_relu(blocks[3].conv1, up2_into(d, buf3)))
        d = self._conv_bn_relu(blocks[4].conv2, self._conv_bn_relu(blocks[4].conv1, up2_cat(d, None)))
        head = self.segmentation_head[0]
        w, b = pad_head(head.weight, head.bias)       # (8-channel granularity: sliced off below)
        return crop_channels(G.conv2d_nhwc(d, w, b), self.out_channels)

    # ---------------------------------------------------------------- the fp32 route (library operations, NCHW)
    def _forward_library(self, x: torch.Tensor) -> torch.Tensor:
        enc = self.encoder
        f1 = enc.relu(enc.bn1(enc.conv1(x)))
        f2 = enc.layer1(enc.maxpool(f1))
        f3 = enc.layer2(f2)
        f4 = enc.layer3(f3)
        d = enc.layer4(f4)
        for blk, skip in zip(self.decoder.blocks, (f4, f3, f2, f1, None)):
            d = blk(d, skip)
        return self.segmentation_head(d)

    # ---------------------------------------------------------------- nn.Module API
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, H, W, in_channels) (or the rollout's zero-padded rows) -> (B, H, W, out_channels); H and W multiples of 32, or any grid
        with ``autopad_enabled``."""
        if self.native:
            L.require_cuda(x)
        H, W = x.shape[1], x.shape[2]
        top, bottom, left, right = self.padding_for(H, W)
        if top or bottom or left or right:
            if not self._settings.autopad_enabled:
                raise L.P4CError(f"CustomUNetMI355X: grid {H}x{W} must be a multiple of 32 in both dimensions (or set autopad_enabled)")
            y = self.forward(F.pad(x, (0, 0, left, right, top, bottom)))
            return y[:, top: top + H, left: left + W, :]
        if x.shape[-1] < self.in_channels:
            raise L.P4CError(f"CustomUNetMI355X: expected {self.in_channels} input channels, got {x.shape[-1]}")
        out_dtype = x.dtype
        x = x.to(self.act_dtype)
        if self.native:
            y = self._forward_native(pad_rows(x, self.cin_pad).contiguous())
        else:
            y = self._forward_library(x[..., : self.in_channels].permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        return cast_out(y, out_dtype)
