"""
UNet on MI355X -- the model behind ``model_name: UNet`` (the reference's config/CLI/model/unet.yaml; registry key ``UNet`` of its
tests/test_models.py).  The reference takes the class from mfai v5.0.1, which is absent here: PARITY UNPINNED; the network is the
well-known brain-segmentation UNet as mfai writes it, restated in tests/unet_reference.py (float64) and checked against that.

With f = ``init_features``: encoder1..4 = block(cin, f 2^k), bottleneck = block(8f, 16f), a 2x2 max-pool in front of encoder2..4 and the
bottleneck; upconv4..1 = ConvTranspose2d(2c, c, 2, stride=2) (with bias); decoder_k = block(2c, c) on cat((upconv_k(.), enc_k), channels);
conv = Conv2d(f, out_channels, 1) (with bias), no final activation.  A block is conv1 (3x3, padding 1, no bias) -> BatchNorm2d -> ReLU
-> conv2 -> BatchNorm2d -> ReLU; state-dict keys follow mfai (``encoder1.enc1conv1.weight``, ``decoder4.dec4norm2.running_mean``, ...).

What runs where, bf16 (``compute_dtype`` / ``activation_dtype`` "bf16"), features-last (B, H, W, C) throughout:
* every 3x3 convolution and the 1x1 head: the implicit-GEMM kernels of csrc/gemm.hip (``ops_gemm.conv2d_nhwc``), with the batch-norm
  statistics from the producer's epilogue; BN + ReLU of the first convolution of every block, of the bottleneck and of the decoders:
  ``ops_gemm.batch_norm_act`` (csrc/inorm.hip);
* the encoder block tail (BN + ReLU of conv2, the skip into the decoder's concatenation buffer, the 2x2 max-pool): ONE pass each way
  (csrc/unet.hip, ``enc_tail``) -- the skip is written straight into the second half of a (B, H, W, 2c) buffer;
* upconv_k: a GEMM with sub-pixel addressing (csrc/gemm.hip, ``p4c_gemm_upconv_*``) whose epilogue stores into the FIRST half of that
  buffer; the decoder's first convolution reads the buffer as its 2c-channel input.  No torch.cat, no max_pool2d, no library
  convolution or GEMM in a training step.
fp32 (the parity flavour): the convolutions and the transposed convolutions run on the library, BN + ReLU and the encoder tails on the
same native passes in fp32 storage.
"""

from dataclasses import dataclass
from collections import OrderedDict
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from . import ops_gemm as G
from .base import ModelType
from .conv_model import ConvModelMI355X, cast_out, crop_channels, pad_head, pad_rows, pad_weight_in

try:
    from dataclasses_json import dataclass_json
except Exception:  # pragma: no cover
    def dataclass_json(cls):
        return cls


@dataclass_json
@dataclass
class UNetSettings:
    """mfai's UNetSettings fields (config/CLI/model/unet.yaml) + the MI355X knobs."""

    init_features: int = 64
    autopad_enabled: bool = False   # mfai's AutoPaddingModel: grids that are not a multiple of 16 are zero-padded (centred) and cropped
    # MI355X-specific
    compute_dtype: str = "f32"      # "f32" (library convolutions, the parity flavour) or "bf16" (the native route)
    activation_dtype: Optional[str] = None   # HBM storage of activations: "f32" | "bf16"; None = compute_dtype


def _block(cin: int, features: int, name: str) -> nn.Sequential:
    return nn.Sequential(OrderedDict([
        (name + "conv1", nn.Conv2d(cin, features, 3, padding=1, bias=False)),
        (name + "norm1", nn.BatchNorm2d(features)),
        (name + "relu1", nn.ReLU(inplace=True)),
        (name + "conv2", nn.Conv2d(features, features, 3, padding=1, bias=False)),
        (name + "norm2", nn.BatchNorm2d(features)),
        (name + "relu2", nn.ReLU(inplace=True)),
    ]))


def _alias(t: torch.Tensor) -> torch.Tensor:
    """a tensor on t's memory with a version counter of its own: the encoder tail keeps the skip values it wrote into the concatenation
    buffer, whose OTHER half the transposed convolution fills in place later (the saved half is never written again)"""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage(), t.storage_offset(), t.shape, t.stride())


class _EncTail(torch.autograd.Function):
    """(buf, pool) = the encoder block's last BN + ReLU written into buf[..., C:] (buf (B, H, W, 2C), its first half left for the
    transposed convolution) and the 2x2 max-pool of it; one native pass each way (csrc/unet.hip) + the batch norm's finalize / apply."""

    @staticmethod
    def forward(ctx, y, stats, gamma, beta, bn, training):
        yc = y.contiguous()
        B, H, W, C = yc.shape
        dev = yc.device
        st = G.bn_statistics(yc, stats, bn, training)
        buf = torch.empty(B, H, W, 2 * C, dtype=yc.dtype, device=dev)
        pool = torch.empty(B, H // 2, W // 2, C, dtype=yc.dtype, device=dev)
        es = yc.element_size()
        L.call("p4c_unet_enc_tail_fwd", L.ptr(yc), L.ptr(st[2]), L.ptr(st[3]), L.ptr(buf[..., C:]), 2 * C, L.ptr(pool), L.dtype_code(yc.dtype),
               B, H, W, C, L.stream(dev), alg_bytes=es * (yc.numel() * 2 + pool.numel()))
        ctx.save_for_backward(yc, st, _alias(buf))
        ctx.training = bool(training)
        ctx.has_affine = gamma is not None
        ctx.set_materialize_grads(False)
        return buf, pool

    @staticmethod
    def backward(ctx, dbuf, dpool):
        yc, st, buf = ctx.saved_tensors
        B, H, W, C = yc.shape
        dev = yc.device
        dbuf = torch.zeros_like(buf) if dbuf is None else dbuf.contiguous()
        dpool = torch.zeros(B, H // 2, W // 2, C, dtype=yc.dtype, device=dev) if dpool is None else dpool.contiguous()
        nb = L.lib().p4c_unet_enc_tail_bwd_blocks(B, H, W, C)
        part = torch.empty(1, nb, 2, C, dtype=torch.float32, device=dev)
        dz = torch.empty_like(yc)
        es = yc.element_size()
        L.call("p4c_unet_enc_tail_bwd", L.ptr(yc), L.ptr(buf[..., C:]), 2 * C, L.ptr(dbuf[..., C:]), 2 * C, L.ptr(dpool), L.ptr(st[0]), L.ptr(st[1]),
               L.ptr(dz), L.ptr(part), L.dtype_code(yc.dtype), B, H, W, C, L.stream(dev), alg_bytes=es * (yc.numel() * 4 + dpool.numel()))
        dy, dg, db = G.bn_tail_backward(yc, dz, part, nb, st, ctx.training, ctx.has_affine)
        return dy, None, dg, db, None, None


def enc_tail(y: torch.Tensor, stats, bn: nn.BatchNorm2d):
    """(buf (B, H, W, 2C) with buf[..., C:] = relu(bn(y)), max_pool2d(relu(bn(y)), 2)) for a features-last y (B, H, W, C), H and W even;
    ``stats``: the producer's column sums or None.  buf[..., :C] is uninitialised: the decoder's transposed convolution fills it."""
    L.require_cuda(y)
    B, H, W, C = y.shape
    if y.dtype not in (torch.float32, torch.bfloat16) or H % 2 or W % 2 or C % 4 or C > 1024:
        raise L.P4CError(f"unet.enc_tail: unsupported map {tuple(y.shape)} {y.dtype}")
    training = bn.training or bn.running_mean is None
    return _EncTail.apply(y, stats if training else None, bn.weight, bn.bias, bn, training)


class _UpConvInto(torch.autograd.Function):
    """buf[..., :Cout] = conv_transpose2d(x, w, b, stride=2) (w (Cin, Cout, 2, 2)) in place, as one GEMM with sub-pixel addressing each
    way (csrc/gemm.hip: p4c_gemm_upconv_fwd / _dgrad / _wgrad); returns buf"""

    @staticmethod
    def forward(ctx, x, w, b, buf, grad_owned):
        xc = x.contiguous()
        B, H, W, Cin = xc.shape
        Cout = w.shape[1]
        dev = xc.device
        fwd = torch.empty(4 * Cout, Cin, dtype=torch.bfloat16, device=dev)
        dgr = torch.empty(Cin, 4 * Cout, dtype=torch.bfloat16, device=dev)
        L.call("p4c_upconv_prep_weight", L.ptr(G._f32(w)), Cin, Cout, L.ptr(fwd), L.ptr(dgr), L.stream(dev))
        M = B * H * W
        nbytes = L.lib().p4c_gemm_nt_workspace_bytes(M, 4 * Cout, Cin)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None
        L.call("p4c_gemm_upconv_fwd", L.ptr(xc), Cin, L.ptr(fwd), L.ptr(G._f32(b)), B, H, W, Cin, Cout, L.ptr(buf), buf.stride(2), L.ptr(ws),
               L.stream(dev), alg_bytes=2 * (M * Cin + 4 * Cout * Cin + 4 * M * Cout), alg_flops=2 * M * 4 * Cout * Cin)
        ctx.mark_dirty(buf)
        ctx.grad_owned = bool(grad_owned)
        ctx.sink = G._sink(w, b)      # (gw, gb) views of the parameters' .grad: the weight gradient is ADDED there (ops_gemm convention)
        ctx.save_for_backward(xc, dgr)
        ctx.meta = (B, H, W, Cin, Cout, buf.stride(2), w.dtype, None if b is None else b.dtype)
        return buf

    @staticmethod
    def backward(ctx, dbuf):
        xc, dgr = ctx.saved_tensors
        B, H, W, Cin, Cout, ld, wdt, bdt = ctx.meta
        dev = xc.device
        dbuf = dbuf.contiguous()
        M = B * H * W
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(B, H, W, Cin, dtype=xc.dtype, device=dev)
            nbytes = L.lib().p4c_gemm_nt_workspace_bytes(M, Cin, 4 * Cout)
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None
            L.call("p4c_gemm_upconv_dgrad", L.ptr(dbuf), ld, L.ptr(dgr), B, H, W, Cin, Cout, L.ptr(dx), Cin, L.ptr(ws), L.stream(dev),
                   alg_bytes=2 * (4 * M * Cout + 4 * Cout * Cin + M * Cin), alg_flops=2 * M * 4 * Cout * Cin)
        dw = db = None
        if ctx.needs_input_grad[1] or (bdt is not None and ctx.needs_input_grad[2]):
            sink = ctx.sink
            if sink is not None:
                dw, db = sink
            else:
                dw = torch.empty(Cin, Cout, 2, 2, dtype=torch.float32, device=dev)
                db = torch.empty(Cout, dtype=torch.float32, device=dev) if bdt is not None else None
            ws = torch.empty(max(L.lib().p4c_gemm_tn_workspace_bytes(M, 4 * Cout, Cin) // 4, 1), dtype=torch.float32, device=dev)
            L.call("p4c_gemm_upconv_wgrad", L.ptr(dbuf), ld, L.ptr(xc), Cin, B, H, W, Cin, Cout, L.ptr(dw), L.ptr(db), int(sink is not None),
                   L.ptr(ws), L.stream(dev), alg_bytes=2 * (4 * M * Cout + M * Cin) + 4 * 4 * Cout * Cin, alg_flops=2 * M * 4 * Cout * Cin)
            if sink is not None:
                L.grad_written(*[t for t in sink if t is not None])
                dw = db = None
            else:
                dw = dw.to(wdt)
                db = None if db is None else db.to(bdt)
        # the forward overwrote channels [:Cout] of buf: their earlier values get no gradient, the other channels' passes through.  In
        # place when the caller says the incoming gradient is this node's alone (the model: the decoder convolution's fresh data gradient)
        if ctx.grad_owned:
            dpass = dbuf
        else:
            dpass = torch.empty_like(dbuf)
            dpass[..., Cout:].copy_(dbuf[..., Cout:])
        dpass[..., :Cout].zero_()
        return dx, dw, db, dpass, None


def upconv_into(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], buf: torch.Tensor, grad_owned: bool = False) -> torch.Tensor:
    """``buf[..., :Cout] = conv_transpose2d(x, w, b, stride=2)`` on features-last bf16 maps (x (B, H, W, Cin), buf (B, 2H, 2W, >= Cout) with
    unit channel stride), in place; returns buf (autograd: buf's earlier channels [:Cout] get a zero gradient, the other channels' gradient
    passes through; with existing fp32 .grad buffers the weight and bias gradients are added there, as ops_gemm's GEMMs do).
    ``grad_owned``: buf's only consumer hands over a gradient tensor nobody else holds, and the backward zeroes its channels [:Cout] in
    place instead of copying the rest"""
    L.require_cuda(x)
    Cin, Cout = w.shape[0], w.shape[1]
    if (x.dtype != torch.bfloat16 or buf.dtype != torch.bfloat16 or w.dtype != torch.float32 or tuple(w.shape[2:]) != (2, 2)
            or Cin % 8 or Cout % 8 or x.shape[-1] != Cin or buf.shape[1] != 2 * x.shape[1] or buf.shape[2] != 2 * x.shape[2]
            or buf.shape[-1] < Cout or buf.stride(-1) != 1 or not buf.is_contiguous()):
        raise L.P4CError(f"unet.upconv_into: unsupported operands (x {tuple(x.shape)} {x.dtype}, w {tuple(w.shape)}, buf {tuple(buf.shape)})")
    return _UpConvInto.apply(x, w, b, buf, bool(grad_owned))


class UNetMI355X(ConvModelMI355X):
    """mfai's UNet (module docstring) on the native kernels of this package."""

    settings_kls = UNetSettings
    model_type = ModelType.CONVOLUTIONAL

    def __init__(self, in_channels: int, out_channels: int, input_shape: tuple = None, settings: UNetSettings = UNetSettings(),
                 *args, **kwargs):
        super().__init__(in_channels, out_channels, input_shape, settings)
        s = settings
        self._resolve_dtypes(s)
        if s.compute_dtype == "bf16" and s.init_features % 8:
            raise ValueError(f"UNetMI355X: the bf16 route needs init_features a multiple of 8 (the GEMM's channel granularity), got "
                             f"{s.init_features}")
        f = s.init_features
        self.encoder1 = _block(in_channels, f, "enc1")
        self.pool1 = nn.MaxPool2d(kernel_size=2, stride=2)
        self.encoder2 = _block(f, f * 2, "enc2")
        self.pool2 = nn.MaxPool2d(kernel_size=2, stride=2)
        self.encoder3 = _block(f * 2, f * 4, "enc3")
        self.pool3 = nn.MaxPool2d(kernel_size=2, stride=2)
        self.encoder4 = _block(f * 4, f * 8, "enc4")
        self.pool4 = nn.MaxPool2d(kernel_size=2, stride=2)
        self.bottleneck = _block(f * 8, f * 16, "bottleneck")
        self.upconv4 = nn.ConvTranspose2d(f * 16, f * 8, kernel_size=2, stride=2)
        self.decoder4 = _block(f * 16, f * 8, "dec4")
        self.upconv3 = nn.ConvTranspose2d(f * 8, f * 4, kernel_size=2, stride=2)
        self.decoder3 = _block(f * 8, f * 4, "dec3")
        self.upconv2 = nn.ConvTranspose2d(f * 4, f * 2, kernel_size=2, stride=2)
        self.decoder2 = _block(f * 4, f * 2, "dec2")
        self.upconv1 = nn.ConvTranspose2d(f * 2, f, kernel_size=2, stride=2)
        self.decoder1 = _block(f * 2, f, "dec1")
        self.conv = nn.Conv2d(f, out_channels, kernel_size=1)
        self.timed_entry_points = ("p4c_gemm_nt", "p4c_gemm_tn", "p4c_unet_enc_tail_fwd", "p4c_unet_enc_tail_bwd", "p4c_gemm_upconv_fwd",
                                   "p4c_gemm_upconv_dgrad", "p4c_gemm_upconv_wgrad", "p4c_inorm_apply")
        self.check_required_attributes()

    def padding_for(self, H: int, W: int):
        """(top, bottom, left, right) zero padding that takes (H, W) to the next multiple of 16 (four 2x2 poolings), centred as mfai's
        AutoPaddingModel does (extra row / column at the end); all zeros when the grid already fits."""
        dh, dw = (-H) % 16, (-W) % 16
        return dh // 2, dh - dh // 2, dw // 2, dw - dw // 2

    # ---------------------------------------------------------------- the two routes of a block
    def _conv(self, m: nn.Conv2d, x: torch.Tensor, want_stats: bool):
        """features-last conv of x; returns (y, stats or None)"""
        if self.native:
            w = m.weight
            if w.shape[1] % 8:          # encoder1 on zero-padded input rows
                w = pad_weight_in(w, x.shape[-1])
            w, b = pad_head(w, m.bias)  # (the head: 8-channel granularity, sliced off below)
            out = G.conv2d_nhwc(x, w, b, want_stats=want_stats)
            y, st = out if want_stats else (out, None)
            return crop_channels(y, m.out_channels), st
        xin = x[..., : m.in_channels] if x.shape[-1] > m.in_channels else x
        y = F.conv2d(xin.permute(0, 3, 1, 2), m.weight, m.bias, padding=m.padding)
        return y.permute(0, 2, 3, 1), None

    def _half_block(self, seq: nn.Sequential, x: torch.Tensor):
        """conv1 -> norm1 -> ReLU -> conv2: (raw conv2 output, its statistics or None)"""
        c1, n1, _, c2, _, _ = seq
        y, st = self._conv(c1, x, True)
        h = G.batch_norm_act(y, st, n1, slope=0.0)
        return self._conv(c2, h, True)

    def _block(self, seq: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
        y, st = self._half_block(seq, x)
        return G.batch_norm_act(y, st, seq[4], slope=0.0)

    def _enc(self, seq: nn.Sequential, x: torch.Tensor):
        y, st = self._half_block(seq, x)
        return enc_tail(y, st, seq[4])

    def _up(self, m: nn.ConvTranspose2d, x: torch.Tensor, buf: torch.Tensor) -> torch.Tensor:
        if self.native:
            return upconv_into(x, m.weight, m.bias, buf, grad_owned=True)   # (the decoder's first convolution is buf's only consumer)
        up = F.conv_transpose2d(x.permute(0, 3, 1, 2), m.weight, m.bias, stride=2).permute(0, 2, 3, 1)
        C = up.shape[-1]
        return torch.cat((up, buf[..., C:]), dim=-1)       # (fp32 flavour only)

    # ---------------------------------------------------------------- nn.Module API
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, H, W, in_channels) (or the rollout's zero-padded rows) -> (B, H, W, out_channels)."""
        L.require_cuda(x)
        H, W = x.shape[1], x.shape[2]
        top, bottom, left, right = self.padding_for(H, W)
        if top or bottom or left or right:
            if not self._settings.autopad_enabled:
                raise L.P4CError(f"UNetMI355X: grid {H}x{W} must be a multiple of 16 in both dimensions (or set autopad_enabled)")
            y = self.forward(F.pad(x, (0, 0, left, right, top, bottom)))
            return y[:, top: top + H, left: left + W, :]
        out_dtype = x.dtype
        if x.shape[-1] < self.in_channels:
            raise L.P4CError(f"UNetMI355X: expected {self.in_channels} input channels, got {x.shape[-1]}")
        x = x.to(self.act_dtype)
        if self.native:
            x = pad_rows(x, self.cin_pad)
        x = x.contiguous()
        buf1, p = self._enc(self.encoder1, x)
        buf2, p = self._enc(self.encoder2, p)
        buf3, p = self._enc(self.encoder3, p)
        buf4, p = self._enc(self.encoder4, p)
        h = self._block(self.bottleneck, p)
        h = self._block(self.decoder4, self._up(self.upconv4, h, buf4))
        h = self._block(self.decoder3, self._up(self.upconv3, h, buf3))
        h = self._block(self.decoder2, self._up(self.upconv2, h, buf2))
        h = self._block(self.decoder1, self._up(self.upconv1, h, buf1))
        y, _ = self._conv(self.conv, h, False)
        return cast_out(y, out_dtype)
