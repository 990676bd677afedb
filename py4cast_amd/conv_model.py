"""What the features-last convolutional models of the registry (UNet, Segformer, DeepLabV3, CustomUNet) share on the host: the plugin attribute
contract, the ``compute_dtype`` / ``activation_dtype`` settings, the rollout's input format, bench.py's roofline hook and the padding
steps that take channel counts to the 8-element granularity of the GEMM kernels (csrc/gemm.hip).  Each model keeps its module tree, its
own settings checks, ``check_grid`` / ``padding_for``, ``timed_entry_points`` and its forward routes."""

from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from .base import ModelABC


def pad_rows(x: torch.Tensor, width: int) -> torch.Tensor:
    """rows off the GEMM's 8-channel granularity zero-padded to ``width`` channels (rows that fit are returned as they are)"""
    return F.pad(x, (0, width - x.shape[-1])) if x.shape[-1] % 8 else x


def pad_weight_in(w: torch.Tensor, cin: int) -> torch.Tensor:
    """a first convolution's (Co, Ci, k, k) weight with zero columns for the padding channels of ``cin``-wide rows"""
    return F.pad(w, (0, 0, 0, 0, 0, cin - w.shape[1])) if w.shape[1] != cin else w


def pad_head(w: torch.Tensor, b: Optional[torch.Tensor]):
    """(w, b) of a head with zero output rows up to the 8-channel granularity; ``crop_channels`` slices the result back (a view)"""
    pad = (-w.shape[0]) % 8
    if not pad:
        return w, b
    return F.pad(w, (0, 0) * (w.dim() - 1) + (0, pad)), None if b is None else F.pad(b, (0, pad))


def crop_channels(y: torch.Tensor, n: int) -> torch.Tensor:
    return y[..., :n] if y.shape[-1] != n else y


def cast_out(y: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """the result in the caller's floating-point dtype"""
    return y if y.dtype == out_dtype or not out_dtype.is_floating_point else y.to(out_dtype)


class ConvModelMI355X(ModelABC, nn.Module):
    """base of the features-last (B, H, W, C) convolutional models: bf16 = the native route, fp32 = the parity flavour on the library"""

    onnx_supported = False
    supported_num_spatial_dims = (2,)
    num_spatial_dims = 2
    features_last = True
    register = True
    is_native_hip = True
    rollout_padded_output = False
    roofline_from_entry_points = True    # bench.py: time every call of the model's timed_entry_points

    def __init__(self, in_channels: int, out_channels: int, input_shape, settings):
        super().__init__()
        self.in_channels, self.out_channels, self.input_shape = in_channels, out_channels, input_shape
        self.num_output_features = out_channels
        self._settings = settings

    def _resolve_dtypes(self, s) -> None:
        """validate ``compute_dtype`` / ``activation_dtype`` and set ``act_dtype``"""
        name = type(self).__name__
        act = s.activation_dtype or s.compute_dtype
        if s.compute_dtype not in ("f32", "bf16") or act not in ("f32", "bf16"):
            raise ValueError(f"{name}: compute_dtype / activation_dtype must be 'f32' or 'bf16', got {s.compute_dtype} / {act}")
        if act != s.compute_dtype:
            raise ValueError(f"{name}: compute_dtype {s.compute_dtype} with activation_dtype {act} is not served: the bf16 route keeps "
                             "bf16 activations, the fp32 route fp32 ones")
        self.act_dtype = torch.bfloat16 if act == "bf16" else torch.float32

    @property
    def settings(self):
        return self._settings

    def roofline(self, ktimes, B, H, W):
        """bench.py: achieved HBM rate of the native entry point that takes the most time"""
        return L.entry_point_roofline(ktimes)

    @property
    def native(self) -> bool:
        """the bf16 route (the kernels of this package); fp32 runs on the library"""
        return self.act_dtype == torch.bfloat16

    @property
    def cin_pad(self) -> int:
        return (self.in_channels + 7) // 8 * 8

    @property
    def rollout_input_format(self):
        """(dtype, channel count) of the rows the rollout's build_x should emit: bf16, zero-padded to the GEMM's 8-channel granularity"""
        if not self.native:
            return None
        return torch.bfloat16, self.cin_pad
