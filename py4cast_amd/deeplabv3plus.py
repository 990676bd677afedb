"""
DeepLabV3+ on MI355X -- the model behind ``model_name: DeepLabV3Plus`` (the reference's config/CLI/model/deeplabv3plus.yaml; registry key
``DeepLabV3Plus`` of its tests/test_models.py).  The reference takes the class from mfai v5.0.1, which wraps
segmentation_models_pytorch's DeepLabV3Plus; neither is installed here: PARITY UNPINNED.  The network is smp's DeepLabV3Plus as its public
documentation and torchvision's ResNet describe it, restated in tests/deeplabv3plus_reference.py (float64) and checked against that.

Assumptions (the architecture as written here):
* encoder (state-dict keys ``encoder.*`` = torchvision's ResNet keys without ``fc``): deeplabv3.ResNetEncoder at output stride 16 (smp's
  make_dilated(output_stride=16)): layer strides (1, 2, 2, 1), layer4's convolutions stride 1 / dilation 2 / padding 2; resnet18 /
  resnet34, ``encoder_depth`` 5.  The decoder reads layer4's output (512 channels, stride 16) and layer1's (64 channels, stride 4: smp's
  ``features[-4]``);
* SeparableConv2d(ci, co, 3, dilation d) = Sequential(``.0`` depthwise Conv2d(ci, ci, 3, padding=d, dilation=d, groups=ci, bias=False),
  ``.1`` pointwise Conv2d(ci, co, 1, bias=False));
* ``decoder.aspp`` = Sequential(ASPP(512, dc, rates 12 / 24 / 36, separable), SeparableConv2d(dc, dc, 3), BN, ReLU), dc =
  decoder_channels; ASPP: convs.0 = 1x1 conv -> BN -> ReLU, convs.1..3 = Sequential(SeparableConv2d(512, dc, 3, d = rate), BN, ReLU),
  convs.4 = AdaptiveAvgPool2d(1) -> 1x1 conv -> BN -> ReLU broadcast over the map, project = 1x1 conv 5 dc -> dc -> BN -> ReLU ->
  Dropout(0.5);
* ``decoder.up`` = UpsamplingBilinear2d(4) (align_corners=True); ``decoder.block1`` = 1x1 conv 64 -> 48 (no bias) -> BN -> ReLU on
  layer1's map; ``decoder.block2`` = Sequential(SeparableConv2d(dc + 48, dc, 3), BN, ReLU) on cat([up(aspp), block1(skip)], channels);
* ``segmentation_head`` = (Conv 1x1 dc -> out with bias, UpsamplingBilinear2d(4)), no activation.  ``upsampling``: the decoder's output is
  at stride 4 and the rollout needs the output on the input's grid (the reference trains this yaml against targets on that grid), so the
  head ALWAYS up-samples x4: ``upsampling`` 4 (smp's default) and 8 (what the shipped yaml passes) both build that head, anything else
  raises;
* initialisation as DeepLabV3's: encoder convs kaiming-normal (fan_out, relu), decoder convs kaiming-uniform (fan_in, relu), head
  xavier-uniform with zero bias, BN weight 1 / bias 0.  ``encoder_weights: True`` never downloads (deeplabv3.load_encoder_weights).

What runs where, bf16 (``compute_dtype`` / ``activation_dtype`` "bf16"), features-last (B, H, W, C) throughout:
* the encoder: DeepLabV3's nodes (``_block`` / ``_patch``); layer2.0 and layer3.0 are strided: patch gather + GEMM, as in CustomUNet;
* every 1x1 convolution (the ASPP's first branch, the pointwise halves, the projection, block1, the head): ``ops_gemm.conv2d_nhwc`` with
  the batch-norm statistics from the GEMM epilogue + ``ops_gemm.batch_norm_act``; the project's Dropout as that pass's multiplier;
* the depthwise halves: csrc/deeplabplus.hip -- the ASPP's three rates from ONE launch each way (``depthwise3x3_dilated``), the same
  kernel at one rate for ``decoder.aspp.1`` and ``decoder.block2.0``;
* the ASPP pooling branch and the projection's 5 dc-wide input: ``deeplabv3.aspp_assemble``;
* ``decoder.up`` + the concatenation with block1's map: one pass each way into the (dc + 48)-wide buffer (``up_cat``);
* the head's x4 up-sampling: ``deeplabv3.upsample_bilinear_ac`` on the head output padded to 8 channels.
No library convolution, GEMM, cat, interpolate, pooling or norm in a training step.
fp32 (the parity flavour): the same network on library operations (NCHW inside); it runs on the CPU too.
"""

from dataclasses import dataclass
from typing import Optional, Sequence

import torch
from torch import nn

from . import _lib as L
from . import ops_gemm as G
from .base import ModelType
from .conv_model import ConvModelMI355X, cast_out, crop_channels, pad_head, pad_rows
from .deeplabv3 import (ASPP_RATES, ENCODER_BLOCKS, ASPPPooling, DeepLabV3MI355X, ResNetEncoder, aspp_assemble, load_encoder_weights, stem_tail,
                        upsample_bilinear_ac)

try:
    from dataclasses_json import dataclass_json
except Exception:  # pragma: no cover
    def dataclass_json(cls):
        return cls


SKIP_CHANNELS = 48          # smp's projection of the stride-4 skip
MAX_RATES = 3               # csrc/deeplabplus.hip: rates per launch


@dataclass_json
@dataclass
class DeepLabV3PlusSettings:
    """mfai's DeepLabV3PlusSettings fields (config/CLI/model/deeplabv3plus.yaml) + the MI355X knobs."""

    encoder_name: str = "resnet18"
    encoder_depth: int = 5
    encoder_weights: bool = True
    decoder_channels: int = 256
    activation: Optional[str] = None
    upsampling: int = 4             # 4 (smp's default) or 8 (the shipped yaml): the head up-samples x4 either way (module docstring)
    aux_params: Optional[dict] = None
    # MI355X-specific
    compute_dtype: str = "f32"      # "f32" (library operations, the parity flavour) or "bf16" (the native route)
    activation_dtype: Optional[str] = None   # HBM storage of activations: "f32" | "bf16"; None = compute_dtype
    aspp_dropout: float = 0.5       # smp's hard-coded p of the ASPP projection's Dropout (0: the parity tests' deterministic network)
    encoder_weights_path: Optional[str] = None   # a torchvision resnet checkpoint (.pth); None: look in torch.hub's checkpoint cache


# ---------------------------------------------------------------- module tree (keys as smp / torchvision)
class SeparableConv2d(nn.Sequential):
    def __init__(self, cin: int, cout: int, dilation: int = 1):
        super().__init__(nn.Conv2d(cin, cin, 3, padding=dilation, dilation=dilation, groups=cin, bias=False),
                         nn.Conv2d(cin, cout, 1, bias=False))


class ASPPSeparableConv(nn.Sequential):
    def __init__(self, cin: int, cout: int, rate: int):
        super().__init__(SeparableConv2d(cin, cout, rate), nn.BatchNorm2d(cout), nn.ReLU())


class SeparableASPP(nn.Module):
    def __init__(self, cin: int, cout: int, rates, dropout: float):
        super().__init__()
        self.convs = nn.ModuleList([nn.Sequential(nn.Conv2d(cin, cout, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU())]
                                   + [ASPPSeparableConv(cin, cout, r) for r in rates] + [ASPPPooling(cin, cout)])
        self.project = nn.Sequential(nn.Conv2d(5 * cout, cout, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(), nn.Dropout(dropout))

    def forward(self, x):
        return self.project(torch.cat([c(x) for c in self.convs], dim=1))


class DeepLabV3PlusDecoder(nn.Module):
    def __init__(self, dc: int, dropout: float):
        super().__init__()
        self.aspp = nn.Sequential(SeparableASPP(512, dc, ASPP_RATES, dropout), SeparableConv2d(dc, dc), nn.BatchNorm2d(dc), nn.ReLU())
        self.up = nn.UpsamplingBilinear2d(scale_factor=4)
        self.block1 = nn.Sequential(nn.Conv2d(64, SKIP_CHANNELS, 1, bias=False), nn.BatchNorm2d(SKIP_CHANNELS), nn.ReLU())
        self.block2 = nn.Sequential(SeparableConv2d(dc + SKIP_CHANNELS, dc), nn.BatchNorm2d(dc), nn.ReLU())

    def forward(self, skip, x):
        """skip: layer1's map (stride 4), x: layer4's (stride 16); NCHW"""
        return self.block2(torch.cat([self.up(self.aspp(x)), self.block1(skip)], dim=1))


# ---------------------------------------------------------------- native nodes
class _DepthwiseDilated(torch.autograd.Function):
    """(y_0, .., y_{R-1}), y_r = depthwise3x3(x; w_r, padding = dilation = d_r): one native launch for the R rates, one for the data
    gradient (the R contributions added in fp32, rounded once), one for the weight-gradient partials + their fixed-order reduction"""

    @staticmethod
    def forward(ctx, x, rates, *ws):
        xc = x.contiguous()
        B, H, W, C = xc.shape
        R = len(ws)
        dev = xc.device
        w32 = torch.empty(R, 9, C, dtype=torch.float32, device=dev)      # tap-major: a tap's weights of a channel octet are 32 contiguous bytes
        for r, w in enumerate(ws):
            w32[r].copy_(w.detach().reshape(C, 9).t())
        ys = [torch.empty_like(xc) for _ in range(R)]
        d3 = tuple(rates) + (1,) * (MAX_RATES - R)
        L.call("p4c_dlp_dw3x3_fwd", L.ptr(xc), L.ptr(w32), *[L.ptr(ys[r]) if r < R else None for r in range(MAX_RATES)], R, *d3, B, H, W, C,
               L.stream(dev), alg_bytes=2 * (1 + R) * xc.numel())
        ctx.save_for_backward(xc, w32)
        ctx.rates, ctx.d3 = tuple(rates), d3
        ctx.wmeta = [(w.shape, w.dtype) for w in ws]
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        xc, w32 = ctx.saved_tensors
        B, H, W, C = xc.shape
        R = len(ctx.rates)
        dev = xc.device
        dys = [g.contiguous() for g in dys]
        gp = [L.ptr(dys[r]) if r < R else None for r in range(MAX_RATES)]
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(xc)
            L.call("p4c_dlp_dw3x3_dgrad", *gp, L.ptr(w32), L.ptr(dx), R, *ctx.d3, B, H, W, C, L.stream(dev), alg_bytes=2 * (1 + R) * xc.numel())
        dws = [None] * R
        if any(ctx.needs_input_grad[2:]):
            rows = L.lib().p4c_dlp_dw3x3_wgrad_rows(B, H, W)
            partial = torch.empty(rows, R * 9 * C, dtype=torch.float32, device=dev)
            L.call("p4c_dlp_dw3x3_wgrad", L.ptr(xc), *gp, L.ptr(partial), R, *ctx.d3, B, H, W, C, L.stream(dev), alg_bytes=2 * 2 * R * xc.numel())
            dw = torch.empty(R, 9, C, dtype=torch.float32, device=dev)
            L.call("p4c_seg_reduce_partials", L.ptr(partial), rows, R * 9 * C, L.ptr(dw), 0, None, 0, L.stream(dev))
            dws = [dw[r].t().reshape(shape).to(dtype) for r, (shape, dtype) in enumerate(ctx.wmeta)]
        return (dx, None, *dws)


def depthwise3x3_dilated(x: torch.Tensor, weights: Sequence[torch.Tensor], rates: Sequence[int]):
    """``[F.conv2d(x, w_r, padding=d_r, dilation=d_r, groups=C) for r]`` (no bias) of a features-last bf16 map x (B, H, W, C), C a
    multiple of 8, for 1 .. 3 fp32 (C, 1, 3, 3) weights and as many rates 1 .. 4095; returns the tuple of the R maps.  One launch reads x
    for all rates; taps outside the map are zero padding (rates beyond the map included)."""
    L.require_cuda(x)
    C = x.shape[-1]
    rates = tuple(rates)
    if (x.dtype != torch.bfloat16 or x.dim() != 4 or C % 8 or not C or not 1 <= len(weights) <= MAX_RATES or len(rates) != len(weights)
            or any(not isinstance(d, int) or not 1 <= d <= 4095 for d in rates)
            or any(tuple(w.shape) != (C, 1, 3, 3) or w.dtype != torch.float32 for w in weights)):
        raise L.P4CError(f"deeplabv3plus.depthwise3x3_dilated: unsupported operands (x {tuple(x.shape)} {x.dtype}, weights "
                         f"{[tuple(w.shape) for w in weights]}, rates {rates}: bf16 (B, H, W, C), C a multiple of 8, 1 .. 3 fp32 (C, 1, 3, 3) "
                         "weights with as many rates 1 .. 4095)")
    return _DepthwiseDilated.apply(x, rates, *weights)


class _UpCat(torch.autograd.Function):
    """out (B, s h, s w, ld) = [bilinear_align_corners_xs(a) | skip | zeros]; one native pass each way"""

    @staticmethod
    def forward(ctx, a, skip, scale, ld):
        ac, sc = a.contiguous(), skip.contiguous()
        B, h, w, Ca = ac.shape
        Cs = sc.shape[-1]
        out = torch.empty(B, scale * h, scale * w, ld, dtype=ac.dtype, device=ac.device)
        L.call("p4c_dlp_up_cat_fwd", L.ptr(ac), L.ptr(sc), L.ptr(out), ld, B, h, w, Ca, Cs, scale, L.stream(ac.device),
               alg_bytes=2 * (ac.numel() + sc.numel() + out.numel()))
        ctx.geom = (B, h, w, Ca, Cs, scale, ld)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, h, w, Ca, Cs, scale, ld = ctx.geom
        dout = dout.contiguous()
        dev = dout.device
        da = torch.empty(B, h, w, Ca, dtype=dout.dtype, device=dev)
        dskip = torch.empty(B, scale * h, scale * w, Cs, dtype=dout.dtype, device=dev)
        L.call("p4c_dlp_up_cat_bwd", L.ptr(dout), ld, L.ptr(da), L.ptr(dskip), B, h, w, Ca, Cs, scale, L.stream(dev),
               alg_bytes=2 * (B * scale * h * scale * w * (Ca + Cs) + da.numel() + dskip.numel()))
        return da, dskip, None, None


def up_cat(a: torch.Tensor, skip: torch.Tensor, scale: int, ld: Optional[int] = None) -> torch.Tensor:
    """``torch.cat([F.interpolate(a, scale_factor=scale, mode="bilinear", align_corners=True), skip], channels)`` of features-last bf16
    maps a (B, h, w, Ca) and skip (B, scale h, scale w, Cs), Ca and Cs multiples of 8, scale 1 .. 8.  ``ld`` (a multiple of 8, >= Ca + Cs;
    default Ca + Cs): the width of the result; its channels from Ca + Cs on are ZEROS.  The up-sampled channels equal
    ``deeplabv3.upsample_bilinear_ac(a, scale)`` bit for bit."""
    L.require_cuda(a, skip)
    ok = all(t.dtype == torch.bfloat16 and t.dim() == 4 and t.shape[-1] and t.shape[-1] % 8 == 0 for t in (a, skip))
    ok = ok and isinstance(scale, int) and 1 <= scale <= 8 and skip.shape[:3] == (a.shape[0], scale * a.shape[1], scale * a.shape[2])
    width = a.shape[-1] + skip.shape[-1]
    ld = width if ld is None else ld
    if not ok or not isinstance(ld, int) or ld < width or ld % 8:
        raise L.P4CError(f"deeplabv3plus.up_cat: unsupported operands (a {tuple(a.shape)} {a.dtype}, skip {tuple(skip.shape)} {skip.dtype}, scale "
                         f"{scale}, ld {ld}: bf16 maps, channel counts multiples of 8, skip on the x scale grid of a, scale 1 .. 8)")
    return _UpCat.apply(a, skip, int(scale), int(ld))


# ---------------------------------------------------------------- the model
class DeepLabV3PlusMI355X(ConvModelMI355X):
    """smp's DeepLabV3Plus as mfai builds it (module docstring) on the native kernels of this package."""

    settings_kls = DeepLabV3PlusSettings
    model_type = ModelType.CONVOLUTIONAL

    def __init__(self, in_channels: int, out_channels: int, input_shape: tuple = None,
                 settings: DeepLabV3PlusSettings = DeepLabV3PlusSettings(), *args, **kwargs):
        super().__init__(in_channels, out_channels, input_shape, settings)
        s = settings
        if s.encoder_name not in ENCODER_BLOCKS:
            raise ValueError(f"DeepLabV3PlusMI355X: encoder_name {s.encoder_name!r} is not served (one of {sorted(ENCODER_BLOCKS)})")
        if s.encoder_depth != 5:
            raise ValueError(f"DeepLabV3PlusMI355X: encoder_depth {s.encoder_depth} is not served (5)")
        if s.decoder_channels <= 0 or s.decoder_channels % 8:
            raise ValueError(f"DeepLabV3PlusMI355X: decoder_channels must be a positive multiple of 8, got {s.decoder_channels}")
        if s.activation is not None:
            raise ValueError(f"DeepLabV3PlusMI355X: activation {s.activation!r} is not served (None: identity)")
        if s.upsampling not in (4, 8):
            raise ValueError(f"DeepLabV3PlusMI355X: upsampling {s.upsampling} is not served (4 or 8: the head up-samples x4 and the output "
                             "has the input's grid)")
        if s.aux_params is not None:
            raise ValueError("DeepLabV3PlusMI355X: aux_params (the classification head) is not served")
        if not 0.0 <= s.aspp_dropout < 1.0:
            raise ValueError(f"DeepLabV3PlusMI355X: aspp_dropout must be in [0, 1), got {s.aspp_dropout}")
        self._resolve_dtypes(s)
        dc = s.decoder_channels
        self.encoder = ResNetEncoder(in_channels, ENCODER_BLOCKS[s.encoder_name], strides=(1, 2, 2, 1), dilations=(1, 1, 1, 2))
        self.decoder = DeepLabV3PlusDecoder(dc, s.aspp_dropout)
        self.segmentation_head = nn.Sequential(nn.Conv2d(dc, out_channels, 1), nn.UpsamplingBilinear2d(scale_factor=4))
        self._init_weights()
        if s.encoder_weights:
            load_encoder_weights(self.encoder, s.encoder_name, in_channels, s.encoder_weights_path, owner="DeepLabV3PlusMI355X")
        self.last_dropout_mask = None      # the bf16 route's last Dropout draw (N, dc) fp32 in {0, 1} (tests)
        # replay 22.07 ms vs eager 22.64 ms per bench step: eager, the host loop (22.3 ms) is as long as the step (profiles/deeplabv3plus_bf16_bench*.json)
        self.prefers_hip_graph = True
        self.timed_entry_points = ("p4c_gemm_nt", "p4c_gemm_tn", "p4c_seg_patch_gather", "p4c_seg_patch_scatter", "p4c_deeplab_stem_fwd",
                                   "p4c_deeplab_stem_bwd", "p4c_deeplab_colsum", "p4c_deeplab_assemble_fwd", "p4c_deeplab_assemble_bwd",
                                   "p4c_deeplab_pool_broadcast", "p4c_dlp_dw3x3_fwd", "p4c_dlp_dw3x3_dgrad", "p4c_dlp_dw3x3_wgrad",
                                   "p4c_dlp_up_cat_fwd", "p4c_dlp_up_cat_bwd", "p4c_upsample_bilinear_ac_fwd", "p4c_upsample_bilinear_ac_bwd",
                                   "p4c_inorm_apply", "p4c_inorm_apply_mul")
        self.check_required_attributes()

    _init_weights = DeepLabV3MI355X._init_weights       # encoder / decoder / head / BN exactly as there
    _patch = staticmethod(DeepLabV3MI355X._patch)       # strided convolution: patch gather + GEMM
    _block = DeepLabV3MI355X._block                     # BasicBlock on the native nodes (strided first blocks through _patch)

    def check_grid(self, H: int, W: int) -> None:
        if H % 16 or W % 16:
            nh, nw = (H + 15) // 16 * 16, (W + 15) // 16 * 16
            raise RuntimeError(f"Wrong input shape height={H}, width={W}. Expected image height and width divisible by 16. Consider pad "
                               f"your images to shape ({nh}, {nw}).")

    # ---------------------------------------------------------------- the bf16 route
    @staticmethod
    def _pointwise(conv: nn.Conv2d, bn: nn.BatchNorm2d, x: torch.Tensor, **kw) -> torch.Tensor:
        y, st = G.conv2d_nhwc(x, conv.weight, want_stats=True)
        return G.batch_norm_act(y, st, bn, slope=0.0, **kw)

    def _separable(self, sep: SeparableConv2d, bn: nn.BatchNorm2d, x: torch.Tensor) -> torch.Tensor:
        (y,) = depthwise3x3_dilated(x, [sep[0].weight], (sep[0].dilation[0],))
        return self._pointwise(sep[1], bn, y)

    def _forward_native(self, x: torch.Tensor) -> torch.Tensor:
        enc, dec = self.encoder, self.decoder
        y, st = self._patch(enc.conv1, x)
        h = stem_tail(y, st, enc.bn1)
        for blk in enc.layer1:
            h = self._block(blk, h)
        skip = h
        for layer in (enc.layer2, enc.layer3, enc.layer4):
            for blk in layer:
                h = self._block(blk, h)
        aspp = dec.aspp[0]
        branches = [self._pointwise(aspp.convs[0][0], aspp.convs[0][1], h)]
        seps = [aspp.convs[k] for k in (1, 2, 3)]
        ys = depthwise3x3_dilated(h, [br[0][0].weight for br in seps], [br[0][0].dilation[0] for br in seps])   # the three rates: one launch
        branches += [self._pointwise(br[0][1], br[1], yr) for br, yr in zip(seps, ys)]
        cat = aspp_assemble(h, branches, aspp.convs[4])
        drop = aspp.project[3]
        if self.training and drop.p > 0:
            keep = 1.0 - drop.p
            mask = torch.empty(cat.numel() // cat.shape[-1], aspp.project[0].weight.shape[0], dtype=torch.float32, device=cat.device).bernoulli_(keep)
            self.last_dropout_mask = mask
            a = self._pointwise(aspp.project[0], aspp.project[1], cat, mul=mask, mul_factor=1.0 / keep)
        else:
            self.last_dropout_mask = None
            a = self._pointwise(aspp.project[0], aspp.project[1], cat)
        a = self._separable(dec.aspp[1], dec.aspp[2], a)
        s = self._pointwise(dec.block1[0], dec.block1[1], skip)
        d = self._separable(dec.block2[0], dec.block2[1], up_cat(a, s, 4))
        head = self.segmentation_head[0]
        w, b = pad_head(head.weight, head.bias)       # (8-channel granularity: sliced off after the up-sampling)
        return crop_channels(upsample_bilinear_ac(G.conv2d_nhwc(d, w, b), 4), self.out_channels)

    # ---------------------------------------------------------------- the fp32 route (library operations, NCHW)
    def _forward_library(self, x: torch.Tensor) -> torch.Tensor:
        enc = self.encoder
        skip = enc.layer1(enc.maxpool(enc.relu(enc.bn1(enc.conv1(x)))))
        return self.segmentation_head(self.decoder(skip, enc.layer4(enc.layer3(enc.layer2(skip)))))

    # ---------------------------------------------------------------- nn.Module API
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, H, W, in_channels) (or the rollout's zero-padded rows) -> (B, H, W, out_channels); H and W multiples of 16."""
        if self.native:
            L.require_cuda(x)
        self.check_grid(x.shape[1], x.shape[2])
        if x.shape[-1] < self.in_channels:
            raise L.P4CError(f"DeepLabV3PlusMI355X: expected {self.in_channels} input channels, got {x.shape[-1]}")
        out_dtype = x.dtype
        x = x.to(self.act_dtype)
        if self.native:
            if self.training and x.shape[0] < 2:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                                 f"{torch.Size([x.shape[0], self._settings.decoder_channels, 1, 1])}")
            y = self._forward_native(pad_rows(x, self.cin_pad).contiguous())
        else:
            y = self._forward_library(x[..., : self.in_channels].permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        return cast_out(y, out_dtype)
