"""Float64 restatement of mfai's Segformer (lucidrains' segformer-pytorch inside, mfai v5.0.1 not on this machine: PARITY UNPINNED),
written as the network is written -- nn.Unfold patch embeddings, einsum attention, torch.cat of the nearest-up-sampled stage maps --
with mfai's state-dict keys.  NCHW in and out.  Assumptions (see py4cast_amd/segformer.py): the final bilinear x8 with
align_corners = False; LayerNorm (x - mean) / (std + eps) g + b over the channels."""
from math import sqrt

import torch
from torch import einsum, nn


class LayerNorm(nn.Module):
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.g = nn.Parameter(torch.ones(1, dim, 1, 1))
        self.b = nn.Parameter(torch.zeros(1, dim, 1, 1))

    def forward(self, x):
        std = torch.var(x, dim=1, unbiased=False, keepdim=True).sqrt()
        mean = torch.mean(x, dim=1, keepdim=True)
        return (x - mean) / (std + self.eps) * self.g + self.b


class PreNorm(nn.Module):
    def __init__(self, dim, fn):
        super().__init__()
        self.fn = fn
        self.norm = LayerNorm(dim)

    def forward(self, x):
        return self.fn(self.norm(x))


class DsConv2d(nn.Module):
    def __init__(self, dim_in, dim_out, kernel_size, padding, stride=1, bias=True):
        super().__init__()
        self.net = nn.Sequential(
            nn.Conv2d(dim_in, dim_in, kernel_size=kernel_size, padding=padding, groups=dim_in, stride=stride, bias=bias),
            nn.Conv2d(dim_in, dim_out, kernel_size=1, bias=bias),
        )

    def forward(self, x):
        return self.net(x)


class EfficientSelfAttention(nn.Module):
    def __init__(self, *, dim, heads, reduction_ratio):
        super().__init__()
        self.scale = (dim // heads) ** -0.5
        self.heads = heads
        self.to_q = nn.Conv2d(dim, dim, 1, bias=False)
        self.to_kv = nn.Conv2d(dim, dim * 2, reduction_ratio, stride=reduction_ratio, bias=False)
        self.to_out = nn.Conv2d(dim, dim, 1, bias=False)

    def forward(self, x):
        h, w = x.shape[-2:]
        heads = self.heads
        q, k, v = (self.to_q(x), *self.to_kv(x).chunk(2, dim=1))
        # rearrange 'b (h c) x y -> (b h) (x y) c'
        q, k, v = (t.reshape(t.shape[0] * heads, t.shape[1] // heads, -1).transpose(1, 2) for t in (q, k, v))
        sim = einsum("b i d, b j d -> b i j", q, k) * self.scale
        attn = sim.softmax(dim=-1)
        out = einsum("b i j, b j d -> b i d", attn, v)
        # rearrange '(b h) (x y) c -> b (h c) x y'
        out = out.transpose(1, 2).reshape(-1, heads * out.shape[-1], h, w)
        return self.to_out(out)


class MixFeedForward(nn.Module):
    def __init__(self, *, dim, expansion_factor):
        super().__init__()
        hidden_dim = dim * expansion_factor
        self.net = nn.Sequential(nn.Conv2d(dim, hidden_dim, 1), DsConv2d(hidden_dim, hidden_dim, 3, padding=1), nn.GELU(),
                                 nn.Conv2d(hidden_dim, dim, 1))

    def forward(self, x):
        return self.net(x)


class MiT(nn.Module):
    def __init__(self, *, channels, dims, heads, ff_expansion, reduction_ratio, num_layers):
        super().__init__()
        stage_kernel_stride_pad = ((7, 4, 3), (3, 2, 1), (3, 2, 1), (3, 2, 1))
        dims = (channels, *dims)
        dim_pairs = list(zip(dims[:-1], dims[1:]))
        self.stages = nn.ModuleList([])
        for (dim_in, dim_out), (kernel, stride, padding), heads_, ff_, r in zip(dim_pairs, stage_kernel_stride_pad, heads, ff_expansion,
                                                                               reduction_ratio):
            get_overlap_patches = nn.Unfold(kernel, stride=stride, padding=padding)
            overlap_patch_embed = nn.Conv2d(dim_in * kernel ** 2, dim_out, 1)
            layers = nn.ModuleList([])
            for _ in range(num_layers):
                layers.append(nn.ModuleList([
                    PreNorm(dim_out, EfficientSelfAttention(dim=dim_out, heads=heads_, reduction_ratio=r)),
                    PreNorm(dim_out, MixFeedForward(dim=dim_out, expansion_factor=ff_)),
                ]))
            self.stages.append(nn.ModuleList([get_overlap_patches, overlap_patch_embed, layers]))

    def forward(self, x):
        h, w = x.shape[-2:]
        layer_outputs = []
        for get_overlap_patches, overlap_embed, layers in self.stages:
            x = get_overlap_patches(x)
            num_patches = x.shape[-1]
            ratio = int(sqrt((h * w) / num_patches))
            x = x.reshape(x.shape[0], x.shape[1], h // ratio, -1)
            x = overlap_embed(x)
            for attn, ff in layers:
                x = attn(x) + x
                x = ff(x) + x
            layer_outputs.append(x)
        return layer_outputs


class SegformerReference(nn.Module):
    def __init__(self, in_channels, out_channels, dims=(32, 64, 160, 256), heads=(1, 2, 5, 8), ff_expansion=(8, 8, 4, 4),
                 reduction_ratio=(8, 4, 2, 1), num_layers=2, decoder_dim=256, num_downsampling_chans=32):
        super().__init__()
        self.downsampler = nn.Conv2d(in_channels, num_downsampling_chans, kernel_size=3, stride=2, padding=1)
        self.mit = MiT(channels=num_downsampling_chans, dims=dims, heads=heads, ff_expansion=ff_expansion, reduction_ratio=reduction_ratio,
                       num_layers=num_layers)
        self.to_fused = nn.ModuleList([nn.Sequential(nn.Conv2d(dim, decoder_dim, 1), nn.Upsample(scale_factor=2 ** i))
                                       for i, dim in enumerate(dims)])
        self.to_segmentation = nn.Sequential(nn.Conv2d(4 * decoder_dim, decoder_dim, 1), nn.Conv2d(decoder_dim, out_channels, 1))
        self.upsample = nn.Upsample(scale_factor=8, mode="bilinear", align_corners=False)

    def forward(self, x):
        x = self.downsampler(x)
        layer_outputs = self.mit(x)
        fused = [to_fused(output) for output, to_fused in zip(layer_outputs, self.to_fused)]
        fused = torch.cat(fused, dim=1)
        return self.upsample(self.to_segmentation(fused))


def reference_from(model, dtype=torch.float64):
    """a SegformerReference with the model's settings and parameters (state dict copied), in `dtype` on the CPU"""
    s = model.settings
    ref = SegformerReference(model.in_channels, model.out_channels, tuple(s.dims), tuple(s.heads), tuple(s.ff_expansion),
                             tuple(s.reduction_ratio), s.num_layers, s.decoder_dim, s.num_downsampling_chans)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return ref.to(dtype)


def ref_forward_nhwc(ref, x):
    """features-last in and out, as the model"""
    return ref(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)


__all__ = ["SegformerReference", "reference_from", "ref_forward_nhwc"]
