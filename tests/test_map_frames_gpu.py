"""
ops.map_planes / ops.map_render (csrc/map_frames.hip) and the native PredictionTimestepPlot / PredictionEpochPlot on the GPU.

map_planes is compared BIT FOR BIT with the reference's fp32 torch expressions evaluated on the CPU
(map_frames_closed_form.planes); map_render with the float64 closed form outside the 2^-13 band around the colour-index
boundaries (map_frames_closed_form.render / compare, where the bounds are derived).
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_frames_closed_form as cf  # noqa: E402

pytestmark = pytest.mark.gpu

H0, W0 = 13, 37   # no multiple of the 256-point tile, of 64 or of 4


def _have_matplotlib():
    try:
        import matplotlib  # noqa: F401

        return True
    except Exception:
        return False


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _equal_or_both_nan(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ------------------------------------------------------------------------------------------------ map_planes
def _planes_case(seed, B, T, spatial, F, mask_kind):
    g = torch.Generator().manual_seed(seed)
    shape = (B, T) + tuple(spatial) + (F,)
    c = {"pred": torch.randn(shape, generator=g), "target": torch.randn(shape, generator=g),
         "std": torch.rand(F, generator=g) * 3 + 0.2, "mean": torch.randn(F, generator=g) * 10, "mask": None, "from_nan": False}
    if mask_kind == "f32":
        c["mask"] = torch.randint(0, 3, shape, generator=g).float() * 0.5      # 0, 0.5, 1: a real product, not a select
    elif mask_kind == "u8":
        c["mask"] = torch.rand(shape, generator=g) > 0.3
    elif mask_kind == "nan":
        c["target"][torch.rand(shape, generator=g) < 0.2] = float("nan")
        c["from_nan"] = True
    return c


def _run_planes(c, dev, features, n, pred=None):
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    if c["from_nan"]:
        spec = ops.MaskSpec(L.MASK_FROM_NAN)
    else:
        spec = ops.MaskSpec.from_tensor(None if c["mask"] is None else c["mask"].to(dev))
    pred = c["pred"].to(dev) if pred is None else pred
    return ops.map_planes(pred, c["target"].to(dev), spec, c["std"].to(dev), c["mean"].to(dev), features, n)


def _check_planes(c, dev, features, n, pred=None):
    planes, vrange = _run_planes(c, dev, features, n, pred)
    want, want_range = cf.planes(c["pred"], c["target"], c["mask"], c["std"], c["mean"], features, n, from_nan=c["from_nan"])
    assert planes.shape == want.shape and vrange.shape == want_range.shape
    assert _same_bits(planes, want), f"planes differ in {int((_bits(planes) != _bits(want)).sum())} elements"
    flat = planes[:, :, :, 0].permute(0, 2, 1, 3).reshape(planes.shape[0], planes.shape[2], -1).cpu()
    assert _equal_or_both_nan(vrange[..., 0], flat.amin(dim=-1)) and _equal_or_both_nan(vrange[..., 1], flat.amax(dim=-1))
    assert _equal_or_both_nan(vrange, want_range)
    return planes, vrange


@pytest.mark.parametrize("T,F,features,mask_kind", [
    (1, 5, (0, 1, 2, 3), "none"), (3, 5, (0, 1, 2, 3), "f32"), (3, 5, (0, 1, 2, 3, 4), "u8"), (3, 5, (4, 1, 3), "nan"),
    (1, 5, (4, 1, 3), "u8"), (3, 21, (0, 1, 2, 3), "none"), (3, 21, (0, 1, 2, 3), "nan"), (1, 21, (20, 7, 0, 13), "f32"),
])
def test_map_planes_equals_the_fp32_restatement_bit_for_bit(T, F, features, mask_kind, gpu_device):
    c = _planes_case(11 + T + F, 3, T, (H0, W0), F, mask_kind)
    planes, vrange = _check_planes(c, gpu_device, features, 2)
    again, vagain = _run_planes(c, gpu_device, features, 2)
    assert _same_bits(planes, again) and _same_bits(vrange, vagain)


def test_map_planes_strided_prediction_and_graph_layout(gpu_device):
    c = _planes_case(5, 3, 3, (H0, W0), 5, "u8")
    big = torch.zeros(3, 5, H0, W0, 5, device=gpu_device)          # the fused rollout hands over a view of a larger buffer
    big[:, 1:4] = c["pred"].to(gpu_device)
    view = big[:, 1:4]
    assert not view.is_contiguous()
    _check_planes(c, gpu_device, (0, 1, 2, 3), 2, pred=view)
    wide = torch.zeros(3, 3, H0, W0, 9, device=gpu_device)          # an inner block that is not dense is copied, not misread
    wide[..., 2:7] = c["pred"].to(gpu_device)
    _check_planes(c, gpu_device, (0, 1, 2, 3), 3, pred=wide[..., 2:7])
    flat = {k: (v.reshape(3, 3, H0 * W0, 5) if isinstance(v, torch.Tensor) and v.dim() == 5 else v) for k, v in c.items()}
    planes, _ = _check_planes(flat, gpu_device, (3, 0), 1)
    assert planes.shape == (1, 3, 2, 2, H0 * W0)


def test_map_planes_past_one_loop_trip(gpu_device):
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    handle = L.lib()
    assert (handle.p4c_map_tile(), handle.p4c_map_max_blocks(), handle.p4c_map_gap()) == (ops.MAP_TILE, ops.MAP_MAX_BLOCKS, ops.MAP_GAP)
    assert (handle.p4c_map_render_pixels(), handle.p4c_map_render_max_blocks()) == (ops.MAP_RENDER_PIXELS, ops.MAP_RENDER_MAX_BLOCKS)
    N = ops.MAP_TILE * (2 * ops.MAP_MAX_BLOCKS + 2) + 5            # every workgroup makes two trips, some a third, the last tile is ragged
    features = (2, 0)
    assert 1 * 1 * len(features) * 2 * N < 2_000_000
    assert handle.p4c_map_planes_workspace_bytes(1, 1, N, len(features)) == ops.MAP_MAX_BLOCKS * len(features) * 2 * 4   # > 1 partial
    c = _planes_case(3, 1, 1, (N,), 3, "f32")
    c["target"][0, 0, N - 2, 2] = 50.0      # the extremes sit in the last, ragged tile and in the first
    c["target"][0, 0, 1, 0] = -50.0
    _, vrange = _check_planes(c, gpu_device, features, 1)
    assert vrange[0, 0, 1].item() == (torch.tensor(50.0) * c["std"][2] + c["mean"][2]).item()
    assert vrange[0, 1, 0].item() == (torch.tensor(-50.0) * c["std"][0] + c["mean"][0]).item()


def test_a_nan_in_the_target_gives_a_nan_range_for_that_feature_only(gpu_device):
    c = _planes_case(8, 3, 3, (H0, W0), 5, "none")
    c["target"][1, 2, 7, 30, 2] = float("nan")
    _, vrange = _check_planes(c, gpu_device, (0, 1, 2, 3), 2)
    isnan = torch.isnan(vrange.cpu())
    want = torch.zeros(2, 4, 2, dtype=torch.bool)
    want[1, 2] = True
    assert torch.equal(isnan, want)


def test_map_ops_check_their_arguments(gpu_device):
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    c = _planes_case(1, 2, 1, (4, 6), 3, "none")
    with pytest.raises(L.P4CError, match="indices"):
        _run_planes(c, gpu_device, (0, 3), 1)
    with pytest.raises(L.P4CError, match="samples"):
        _run_planes(c, gpu_device, (0,), 3)
    planes, vrange = _run_planes(c, gpu_device, (0, 1), 2)
    lut, interior = torch.zeros(256, 3, dtype=torch.uint8, device=gpu_device), torch.ones(24, device=gpu_device)
    with pytest.raises(L.P4CError, match="grid"):
        ops.map_render(planes, vrange, lut, interior, 5, 5)
    with pytest.raises(L.P4CError, match="colour table"):
        ops.map_render(planes, vrange, lut[:, :2], interior, 4, 6)


# ------------------------------------------------------------------------------------------------ map_render
def _render_case(seed, n, T, K, H, W, special=True):
    g = torch.Generator().manual_seed(seed)
    planes = torch.randn(n, T, K, 2, H * W, generator=g) * 3 + 1
    if special:
        planes[0, :, 1, 0] = 2.5                                  # a constant target: vmax == vmin, x = 0 in both panels
        planes[0, 0, 2, 0, 5] = float("nan")                      # a NaN pixel in a panel whose range is finite (set below)
        planes[0, 0, 2, 1, 17] = float("nan")
    flat = planes[:, :, :, 0].permute(0, 2, 1, 3).reshape(n, K, -1)
    vrange = torch.stack([torch.nan_to_num(flat, nan=0.0).amin(dim=-1), torch.nan_to_num(flat, nan=0.0).amax(dim=-1)], dim=-1)
    if special:
        vrange[n - 1, 0, 1] = float("nan")                        # a NaN range: both panels white
    return planes, vrange


def _render(planes, vrange, lut, interior, H, W, dev):
    from py4cast_amd import ops

    frames = ops.map_render(planes.to(dev), vrange.to(dev), torch.from_numpy(lut).to(dev), torch.from_numpy(interior).to(dev).reshape(-1), H, W)
    return frames.cpu().numpy()


@pytest.mark.parametrize("H,W,seed", [(13, 37, 1), (64, 64, 2)])
def test_map_render_against_the_float64_closed_form(H, W, seed, gpu_device):
    from py4cast_amd import ops

    assert ops.MAP_GAP == cf.GAP
    planes, vrange = _render_case(seed, 2, 2, 3, H, W)
    lut, interior = cf.synthetic_lut(), cf.border_interior(H, W, 2)
    want = cf.render(planes.numpy(), vrange.numpy(), lut, interior, H, W)
    got = _render(planes, vrange, lut, interior, H, W, gpu_device)
    share = cf.compare(got, want)
    print(f"render {H}x{W}: band share {share:.3e}")
    assert share <= 1e-3
    # the layout, spelled out: gap columns, the white fills, the flip, the panel order
    assert (got[..., W:W + cf.GAP, :] == 255).all()
    assert (got[1, :, 0] == 255).all()                                            # NaN range
    r5, c5 = H - 1 - 5 // W, 5 % W
    assert (got[0, 0, 2, r5, c5] == 255).all()                                    # NaN pixel, target panel
    r17, c17 = H - 1 - 17 // W, 17 % W
    assert (got[0, 0, 2, r17, W + cf.GAP + c17] == 255).all()                     # NaN pixel, prediction panel
    assert (got[0, :, 1, 2:H - 2, 2:W - 2] == lut[0]).all()                       # constant target: index 0, interior
    inside = ~want["band"] & ~want["white"]
    r, c = H - 1 - 6, 9                                                            # grid point (6, 9): interior
    for panel, col in ((0, c), (1, W + cf.GAP + c)):
        if inside[1, 1, 1, r, col]:
            assert got[1, 1, 1, r, col, 0] == want["index"][1, 1, 1, panel, r, c]  # channel 0 of the table is the index


def test_map_render_past_one_loop_trip(gpu_device):
    from py4cast_amd import ops

    n, T, K, H, W = 1, 2, 4, 128, 256
    per_trip = ops.MAP_RENDER_MAX_BLOCKS * 256 * ops.MAP_RENDER_PIXELS
    assert per_trip < n * T * K * H * (2 * W + ops.MAP_GAP) < 2 * per_trip and n * T * K * 2 * H * W < 2_000_000
    planes, vrange = _render_case(4, n, T, K, H, W, special=False)
    lut, interior = cf.synthetic_lut(), cf.border_interior(H, W, 2)
    got = _render(planes, vrange, lut, interior, H, W, gpu_device)
    share = cf.compare(got, cf.render(planes.numpy(), vrange.numpy(), lut, interior, H, W))
    print(f"render {H}x{W}: band share {share:.3e}")
    assert share <= 1e-3


def test_map_render_odd_pixel_count_and_equal_bits(gpu_device):
    """13 x 37 with one frame: 1066 pixels, two left over after the 4-pixel groups; they leave as single bytes"""
    planes, vrange = _render_case(6, 1, 1, 1, H0, W0, special=False)
    lut, interior = cf.synthetic_lut(), cf.border_interior(H0, W0, 2)
    assert (H0 * (2 * W0 + cf.GAP)) % 4 == 2
    got = _render(planes, vrange, lut, interior, H0, W0, gpu_device)
    assert cf.compare(got, cf.render(planes.numpy(), vrange.numpy(), lut, interior, H0, W0)) <= 1e-3
    assert np.array_equal(got, _render(planes, vrange, lut, interior, H0, W0, gpu_device))


@pytest.mark.skipif(not _have_matplotlib(), reason="matplotlib's own colour mapping is the reference here")
def test_interior_pixels_equal_matplotlibs_plasma(gpu_device):
    from matplotlib import colormaps
    from matplotlib.colors import Normalize

    from py4cast_amd.observers import plasma_table

    H, W = 64, 64
    planes, vrange = _render_case(2, 2, 2, 3, H, W, special=False)
    lut, interior = plasma_table(), cf.border_interior(H, W, 2)
    got = _render(planes, vrange, lut, interior, H, W, gpu_device)
    want = cf.render(planes.numpy(), vrange.numpy(), lut, interior, H, W)
    keep = ~want["band"] & want["exact"]
    for s in range(2):
        for k in range(3):
            norm = Normalize(vmin=float(vrange[s, k, 0]), vmax=float(vrange[s, k, 1]))
            for t in range(2):
                for panel, c0 in ((0, 0), (1, W + cf.GAP)):
                    v = planes[s, t, k, panel].numpy().reshape(H, W)[::-1]
                    rgb = colormaps["plasma"](norm(v), bytes=True)[..., :3]
                    m = keep[s, t, k, :, c0:c0 + W]
                    assert np.array_equal(got[s, t, k, :, c0:c0 + W][m], rgb[m])


# ------------------------------------------------------------------------------------------------ observers and Lightning
class Experiment:
    def __init__(self):
        self.figures = []

    def add_scalar(self, name, value, step):
        pass

    def add_figure(self, name, fig, step):
        self.figures.append((name, fig, int(step)))


def _module(gpu_device, tmp_path, exp, case):
    from helpers import make_dataset_info, register_test_models
    from py4cast_amd.lightning import AutoRegressiveLightning

    register_test_models()
    info = make_dataset_info(case, Ff=5)
    info.shortnames.setdefault("output", [])
    lm = AutoRegressiveLightning({}, info, None, num_input_steps=1, num_pred_steps_train=3, num_pred_steps_val_test=3, batch_size=2,
                                 model_name="TinyConvModel")
    lm = lm.to(gpu_device)
    lm.trainer = types.SimpleNamespace(logger=types.SimpleNamespace(log_dir=str(tmp_path), experiment=exp), precision="32-true")
    lm.log_dict = lambda d, **kw: None
    with pytest.warns(UserWarning):
        lm.setup("test")
    return lm, info


def _files(root, sub):
    d = root / sub
    return sorted(p.name for p in d.iterdir()) if d.exists() else []


def test_validation_and_test_steps_write_the_reference_file_names(gpu_device, tmp_path):
    from helpers import make_batch, synthetic_case
    from PIL import Image

    from py4cast_amd import observers, ops
    from py4cast_amd.observers import PredictionEpochPlot, PredictionTimestepPlot

    H, W, T = 16, 24, 3
    case = synthetic_case(seed=5, B=2, T=T, H=H, W=W, F=3, border=2)
    exp = Experiment()
    lm, info = _module(gpu_device, tmp_path, exp, case)
    names = info.shortnames["input_output"]
    lut = None if _have_matplotlib() else cf.synthetic_lut()      # without matplotlib the GIF is still written from a table
    calls = {"planes": 0, "render": 0}
    map_planes, map_render = ops.map_planes, ops.map_render
    observers.ops.map_planes = lambda *a, **k: (calls.__setitem__("planes", calls["planes"] + 1), map_planes(*a, **k))[1]
    observers.ops.map_render = lambda *a, **k: (calls.__setitem__("render", calls["render"] + 1), map_render(*a, **k))[1]
    try:
        lm.on_validation_start()
        assert [type(p) for p in lm.valid_map_plotters] == [PredictionTimestepPlot, PredictionEpochPlot]
        for p in lm.valid_map_plotters:
            p._lut_host = lut if lut is not None else p._lut_host
        lm.validation_step(make_batch(case, gpu_device), 0)
        assert calls == {"planes": 2, "render": 2}                # one of each per plotter
        lm.validation_step(make_batch(case, gpu_device), 1)       # num_samples_to_plot = 1 is reached: nothing more
        assert calls == {"planes": 2, "render": 2} and [p.plotted_examples for p in lm.valid_map_plotters] == [1, 1]
        gifs = [f"{v}.gif" for v in names]
        pngs = [f"{v}_example_1_{t}.png" for v in names for t in range(1, T + 1)] if _have_matplotlib() else []
        assert _files(tmp_path, "timestep_evol_per_param") == sorted(gifs + pngs)
        assert _files(tmp_path, "epoch_evol_per_param") == (sorted(f"{v}_example_1_0.png" for v in names) if _have_matplotlib() else [])
        for v in names:
            with Image.open(tmp_path / "timestep_evol_per_param" / f"{v}.gif") as gif:
                assert gif.n_frames == T and gif.size == (2 * W + ops.MAP_GAP, H)       # PIL: (width, height)
        if _have_matplotlib():
            want = [(f"timestep_evol_per_param/{v}_example_1", t) for t in range(1, T + 1) for v in names]
            want += [(f"epoch_evol_per_param/{v}_example_1", 0) for v in names]
            assert [(f[0], f[2]) for f in exp.figures if "_evol_per_param/" in f[0]] == want
            titles = [f[1]._suptitle.get_text() for f in exp.figures if f[0].startswith("timestep_evol")]
            assert titles[0] == f"{names[0]} (), t=1 ({observers.MapPlot.pred_step(lm) * 1} h)"
        # a second epoch, off the plot period: nothing is built anew, nothing is written
        before = {p: p.stat().st_mtime_ns for p in tmp_path.rglob("*") if p.is_file()}
        n_figures = len(exp.figures)
        lm.trainer.current_epoch = 1
        try:
            lm.current_epoch = 1
        except AttributeError:      # a LightningModule reads the trainer's
            pass
        lm.on_validation_start()
        lm.validation_step(make_batch(case, gpu_device), 0)
        assert calls == {"planes": 2, "render": 2} and len(exp.figures) == n_figures
        assert {p: p.stat().st_mtime_ns for p in tmp_path.rglob("*") if p.is_file()} == before
        # the test step: PredictionTimestepPlot alone, num_samples_to_plot of the module
        for p in tmp_path.rglob("*"):
            if p.is_file():
                p.unlink()
        lm.on_test_start()
        assert [type(p) for p in lm.test_map_plotters] == [PredictionTimestepPlot]
        assert lm.test_map_plotters[0].num_samples_to_plot == lm.num_samples_to_plot and lm.test_map_plotters[0].prefix == "Test"
        lm.test_map_plotters[0]._lut_host = lut if lut is not None else lm.test_map_plotters[0]._lut_host
        lm.test_step(make_batch(case, gpu_device), 0)
        assert calls == {"planes": 3, "render": 3}
        assert _files(tmp_path, "timestep_evol_per_param") == sorted(gifs + pngs) and _files(tmp_path, "epoch_evol_per_param") == []
        assert lm.test_map_plotters[0].plotted_examples == min(2, lm.num_samples_to_plot)
    finally:
        observers.ops.map_planes, observers.ops.map_render = map_planes, map_render


def test_observer_frames_equal_the_ops_and_the_graph_layout_unfolds(gpu_device, tmp_path):
    """the frames a plotter composes from are map_render's of map_planes' on the very tensors, for two samples of a NaN-masked
    batch in the graph layout (B,T,N,F), with units, a step duration and two of three variables"""
    from py4cast_amd import ops
    from py4cast_amd.base import Stats
    from py4cast_amd.losses import NanMask
    from py4cast_amd.namedtensor import NamedTensor
    from py4cast_amd.observers import PredictionEpochPlot, PredictionTimestepPlot

    B, T, F = 3, 2, 3
    c = _planes_case(21, B, T, (H0 * W0,), F, "nan")
    names = ["t2m", "u10", "r"]
    lut, interior = cf.synthetic_lut(), torch.from_numpy(cf.border_interior(H0, W0, 2)).to(gpu_device)
    info = types.SimpleNamespace(units={"t2m": "K", "u10": "m/s", "r": "%"}, pred_step=3)
    stats = Stats({v: {"std": c["std"][i], "mean": c["mean"][i]} for i, v in enumerate(names)})
    exp = Experiment()
    obj = types.SimpleNamespace(dataset_info=info, stats=stats, interior_2d=interior[:, :, None], grid_shape=(H0, W0), current_epoch=4,
                                trainer=types.SimpleNamespace(is_global_zero=True, logger=types.SimpleNamespace(experiment=exp)))
    dims = ["batch", "timestep", "ngrid", "features"]
    raw = c["target"].to(gpu_device)
    pred, target = NamedTensor(c["pred"].to(gpu_device), dims, names), NamedTensor(raw, dims, names)
    seen = []
    for cls in (PredictionTimestepPlot, PredictionEpochPlot):
        plotter = cls(num_samples_to_plot=2, num_features_to_plot=2, prefix="Test", save_path=tmp_path, lut=lut)
        plotter.plot_map = lambda o, frames, vrange, nm, seen=seen: seen.append((frames.copy(), vrange.copy(), list(nm)))
        plotter.update(obj, None, pred, target, NanMask(raw))
        assert plotter.plotted_examples == 2
        plotter.update(obj, None, pred, target, NanMask(raw))
        assert plotter.plotted_examples == 2
    assert len(seen) == 4 and all(s[2] == names[:2] for s in seen)
    want, want_range = cf.planes(c["pred"], c["target"], None, c["std"], c["mean"], (0, 1), 2, from_nan=True)
    frames = ops.map_render(want.to(gpu_device), want_range.to(gpu_device), torch.from_numpy(lut).to(gpu_device), interior.reshape(-1),
                            H0, W0).cpu().numpy()
    for s in range(2):
        assert np.array_equal(seen[s][0], frames[s]) and np.array_equal(seen[s][1], want_range[s].numpy())
        assert np.array_equal(seen[2 + s][0], frames[s, -1:]) and np.array_equal(seen[2 + s][1], want_range[s].numpy())
