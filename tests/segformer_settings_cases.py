"""
The four non-default Segformer configurations of tests/test_segformer_settings_bf16_gpu.py (the device) and
tests/test_segformer_settings_cpu.py (the device-free half): the table, the seeds, the initialisation and the inputs, so that both files
build the same networks.  Test infrastructure, not collected.

What each row is for (keys per stage = the number of keys / values the attention core sees, (H / 2^(s+3) / r)(W / 2^(s+3) / r)):
* narrow  the smallest widths the bf16 route admits next to the 32-wide heads: FFN widths 32, 64, 64, 96 (expansions 1 and 2), an
          8-channel downsampler in front of the 7 x 7 embedding, decoder_dim 64, 5 -> 3 channels (both padded), ONE layer per stage,
          8 / 8 / 8 / 2 keys: masked tails of the 32-key chunk at every stage;
* wide    dims up to the LayerNorm's 512 and 16 heads, THREE layers, reduction ratio 16 (one key per sample: 2-row key / value GEMMs
          over 64 * 256 columns -- 1 row here, B = 1), decoder_dim 128, a 64-channel downsampler;
* tails   the default widths with reduction ratios (1, 2, 1, 1) on 64 x 192: 192 keys (six whole chunks), 12, 12 and 3;
* cap     reduction ratio 1 everywhere on 128 x 128: 256 keys at stage 1, the most the bf16 route serves; 8 -> 64 channels, no padding
          at either end.

Initialisation: torch's default under ``torch.manual_seed(SEED)``, the LayerNorm parameters moved by 0.1 N(0, 1) as
tests/test_segformer_nodes_gpu.py does.  The block checks hold a block's own part (y - x) to 3e-2 and need it to be at least 0.05 of x to
mean anything: a condition on the inputs, asserted in float64 on the CPU (test_segformer_settings_cpu.py), never a measurement of the
kernels.  With this seed it holds without any scale on the blocks' last projections: the smallest own part is 0.195 of x in `narrow`
(its expansion-1 Mix-FFN included), 0.086 in `wide` (the third layer of stage 4), 0.102 in `tails` and 0.104 in `cap`.
"""
import torch

SEED = 0

DEFAULT = dict(dims=(32, 64, 160, 256), heads=(1, 2, 5, 8), ff_expansion=(8, 8, 4, 4), num_layers=2, decoder_dim=256, num_downsampling_chans=32)

CASES = {
    "narrow": dict(dims=(32, 32, 64, 96), heads=(1, 1, 2, 3), ff_expansion=(1, 2, 1, 1), reduction_ratio=(4, 2, 1, 1), num_layers=1,
                   decoder_dim=64, num_downsampling_chans=8, cin=5, cout=3, B=3, grid=(64, 128), keys=(8, 8, 8, 2), hidden=(32, 64, 64, 96)),
    "wide": dict(dims=(64, 128, 320, 512), heads=(2, 4, 10, 16), ff_expansion=(4, 4, 2, 2), reduction_ratio=(16, 2, 2, 1), num_layers=3,
                 decoder_dim=128, num_downsampling_chans=64, cin=69, cout=60, B=1, grid=(128, 128), keys=(1, 16, 4, 4),
                 hidden=(256, 512, 640, 1024)),
    "tails": dict(DEFAULT, reduction_ratio=(1, 2, 1, 1), cin=21, cout=12, B=2, grid=(64, 192), keys=(192, 12, 12, 3),
                  hidden=(256, 512, 640, 1024)),
    "cap": dict(DEFAULT, reduction_ratio=(1, 1, 1, 1), cin=8, cout=64, B=2, grid=(128, 128), keys=(256, 64, 16, 4),
                hidden=(256, 512, 640, 1024)),
}
NAMES = list(CASES)
SETTING_FIELDS = ("dims", "heads", "ff_expansion", "reduction_ratio", "num_layers", "decoder_dim", "num_downsampling_chans")


def settings_of(name, key):
    from py4cast_amd.segformer import SegformerSettings

    c = CASES[name]
    return SegformerSettings(**{f: c[f] for f in SETTING_FIELDS}, compute_dtype=key, activation_dtype=key)


def make_model(name, key, dev="cpu"):
    """the configuration's SegformerMI355X in the flavour ``key`` ("f32" | "bf16") with the initialisation of the module docstring"""
    from py4cast_amd.segformer import SegformerMI355X

    c = CASES[name]
    torch.manual_seed(SEED)
    m = SegformerMI355X(c["cin"], c["cout"], c["grid"], settings_of(name, key))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("norm.g") or n.endswith("norm.b"):
                p.add_(0.1 * torch.randn_like(p))
    return m.to(dev)


def make_inputs(name, dev="cpu"):
    """(x (B, H, W, cin), dy (B, H, W, cout)) fp32, drawn on the CPU so that every device sees the same numbers"""
    c = CASES[name]
    g = torch.Generator().manual_seed(SEED + 1)
    x = torch.randn(c["B"], *c["grid"], c["cin"], generator=g)
    dy = torch.randn(c["B"], *c["grid"], c["cout"], generator=g)
    return x.to(dev), dy.to(dev)


def assert_case_shapes(name, model=None):
    """the row really is what the table says: key counts by check_grid's arithmetic (H / 2^(s+3) / r)(W / 2^(s+3) / r), FFN widths
    dims x ff_expansion, no grid above 128 x 192 -- from the table's settings, and from the built model's own ratios and modules"""
    c = CASES[name]
    H, W = c["grid"]
    keys = tuple((H // (8 << s) // r) * (W // (8 << s) // r) for s, r in enumerate(c["reduction_ratio"]))
    hidden = tuple(d * f for d, f in zip(c["dims"], c["ff_expansion"]))
    assert keys == c["keys"] and hidden == c["hidden"] and H <= 128 and W <= 192, (name, keys, hidden)
    if model is not None:
        keys = tuple((H // (8 << s) // r) * (W // (8 << s) // r) for s, r in enumerate(model.ratios))
        hidden = tuple(stage[2][0][1].fn.net[0].out_channels for stage in model.mit.stages)
        assert keys == c["keys"] and hidden == c["hidden"], (name, keys, hidden)
        assert all(len(stage[2]) == c["num_layers"] for stage in model.mit.stages)
