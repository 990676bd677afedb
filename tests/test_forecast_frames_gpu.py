"""
ops.forecast_frames (csrc/forecast_frames.hip), the GIF writer and predict_step / Trainer.predict with ``io_conf`` on the GPU.

The kernel's ranges and bad mask are compared BIT FOR BIT with the fp32 restatement (forecast_frames_closed_form.values), its
palette indices with the float64 closed form outside the 2^-13 band around the index boundaries (indices / compare, where the bound
is derived; tests/test_forecast_frames_cpu.py proves the closed form against matplotlib and bounds the band's share on the same
cases).
"""
import ctypes
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forecast_frames_closed_form as cf  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _run(c, dev, pred=None, out=None):
    from py4cast_amd import ops

    pred = c["pred"].to(dev) if pred is None else pred
    return ops.forecast_frames(pred, c["std"].to(dev), c["mean"].to(dev), c["display"], samples=c["samples"], features=c["features"], out=out)


def _check(c, dev, pred=None):
    (v, bad, vrange), want = cf.expected(c)
    frames, got_range = _run(c, dev, pred)
    assert got_range.shape == vrange.shape and torch.equal(_bits(got_range), _bits(vrange)), "the colour ranges differ in their bits"
    got = frames.cpu().numpy()
    assert np.array_equal(got == cf.BAD, want["bad"])
    share = cf.compare(got, want)
    again, range_again = _run(c, dev, pred)
    assert torch.equal(frames, again) and torch.equal(_bits(got_range), _bits(range_again))
    return got, want, share


@pytest.fixture(scope="module")
def forms():
    from py4cast_amd import _lib as L

    return lambda K, F: bool(L.lib().p4c_forecast_frames_dense(K, F))


@pytest.mark.parametrize("name", sorted(cf.SHAPES))
def test_frames_against_the_closed_form(name, gpu_device, forms):
    B, T, H, W, F, samples, features = cf.SHAPES[name]
    K = F if features is None else len(features)
    assert forms(K, F) == (name != "e")                # a .. d transpose whole points through LDS, e gathers
    c = cf.case(name)
    got, want, share = _check(c, gpu_device)
    print(f"forecast frames {name}: band share {share:.3e}")
    n = B if samples is None else len(samples)
    assert got.shape == (n, T, K, H, W)
    # the planted frames of the third drawn feature, spelled out: all NaN, constant, one good pixel
    assert (got[0, 0, 2] == cf.BAD).all()
    assert (got[0, 1, 2] == 0).all()
    s, t = (1, 0) if T == 2 else (0, 2)
    one = got[s, t, 2]
    y, x = divmod((H * W) // 3, W)
    assert one[H - 1 - y, x] == 0 and (one == cf.BAD).sum() == H * W - 1
    # the first drawn feature: exactly vmin -> 0, exactly vmax and beyond -> 254, one ulp below the floor -> bad (point 7 i + 3)
    first = got[0, 0, 0]
    at = lambda i: first[H - 1 - ((7 * i + 3) % (H * W)) // W, ((7 * i + 3) % (H * W)) % W]  # noqa: E731
    assert [at(i) for i in range(7)] == [0, 254, 254, 0, 0, cf.BAD, 254]


def test_a_strided_view_of_a_larger_buffer(gpu_device):
    """the native rollout hands over ``states[:, T_in:]``: a batch stride larger than T*N*F"""
    c = cf.case("a")
    B, T, H, W, F = c["pred"].shape
    big = torch.full((B, T + 2, H, W, F), 7.0, device=gpu_device)
    big[:, 2:] = c["pred"].to(gpu_device)
    view = big[:, 2:]
    assert not view.is_contiguous() and view.stride(0) > T * H * W * F
    _check(c, gpu_device, pred=view)
    wide = torch.zeros(B, T, H, W, F + 3, device=gpu_device)      # an inner block that is not dense is copied, not misread
    wide[..., 1:F + 1] = c["pred"].to(gpu_device)
    _check(c, gpu_device, pred=wide[..., 1:F + 1])


@pytest.mark.parametrize("form", ["dense", "gather"])
def test_past_one_loop_trip_of_every_launch(form, gpu_device, forms):
    """the smallest grid that sends a workgroup of the range launch and of the index launch through a second trip, from the
    library's own launch arithmetic; the finish launch reads more than one partial per frame"""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    handle = L.lib()
    tile, cap = handle.p4c_forecast_tile(), handle.p4c_forecast_max_blocks()
    assert (tile, cap, handle.p4c_forecast_max_features(), handle.p4c_forecast_max_samples()) == (
        ops.FORECAST_TILE, ops.FORECAST_MAX_BLOCKS, ops.FORECAST_MAX_FEATURES, ops.FORECAST_MAX_SAMPLES)
    B, T, H, W = cf.LOOP_SHAPE
    F, features = cf.LOOP_FEATURES[form]
    per_pair = cap // (B * T)                                      # workgroups of one (sample, lead time)
    N = H * W
    tiles = -(-N // tile)
    assert per_pair < tiles <= 2 * per_pair and N % tile and N % 4        # a second trip for some, a ragged last tile, a byte tail
    assert handle.p4c_forecast_frames_workspace_bytes(B, T, N, len(features)) == B * T * per_pair * len(features) * 2 * 4
    assert forms(len(features), F) == (form == "dense")
    c = cf.loop_case(form)
    got, want, share = _check(c, gpu_device)
    print(f"forecast frames past one trip ({form}): band share {share:.3e}")
    _, vrange = _run(c, gpu_device)
    off = np.float32(-273.15)
    assert vrange[1, 1, 1, 1].item() == float(np.float32(np.float32(50.0 * 5.0) + np.float32(280.0)) + off)
    assert vrange[1, 1, 1, 0].item() == float(np.float32(np.float32(-50.0 * 5.0) + np.float32(280.0)) + off)


def test_given_ranges_only_is_one_launch(gpu_device, monkeypatch):
    """no drawn feature auto-scales: no workspace, and vrange holds the given ranges"""
    from py4cast_amd import _lib as L

    c = cf.case("b")
    c["features"] = (0, 2, 4)
    c["display"][0] = (None, -5.0, -3.0, 5.0)
    c["display"][2] = (None, None, -1.0, 1.0)
    seen = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a, **k: (seen.append((name, a)), real(name, *a, **k))[1])
    (v, bad, vrange), want = cf.expected(c)
    frames, got_range = _run(c, gpu_device)
    (name, args), = seen
    assert name == "p4c_forecast_frames" and args[8] == 0 and args[11] is None       # auto_range, workspace
    assert torch.equal(_bits(got_range), _bits(vrange))
    cf.compare(frames.cpu().numpy(), want)


def test_bad_arguments_return_the_code_and_launch_nothing(gpu_device):
    from py4cast_amd import _lib as L

    handle = L.lib()
    B, T, H, W, F, K = 2, 1, 4, 8, 3, 3
    dev = gpu_device
    pred = torch.randn(B, T, H, W, F, device=dev)
    std, mean = torch.ones(F, device=dev), torch.zeros(F, device=dev)
    feats = torch.arange(K, dtype=torch.int32, device=dev)
    rows = torch.tensor([[0.0, -cf.INF, cf.NAN, cf.NAN]] * K, dtype=torch.float32, device=dev)
    frames = torch.full((B * T * K * H * W + 8,), 0xA5, dtype=torch.uint8, device=dev)
    vrange = torch.full((B, T, K, 2), -777.0, device=dev)
    ws = torch.empty(handle.p4c_forecast_frames_workspace_bytes(B, T, H * W, K) // 4 + 1, device=dev)
    stream = L.stream(dev)

    def call(pred_=pred, samples=(0, 1), std_=std, frames_=frames, ws_=ws, n=B, K_=K, H_=H, W_=W, T_=T):
        host = (ctypes.c_int32 * len(samples))(*samples)
        return handle.p4c_forecast_frames(L.ptr(pred_), T * H * W * F, H * W * F, host, L.ptr(std_), L.ptr(mean), L.ptr(feats), L.ptr(rows), 1,
                                          ctypes.c_void_p(frames_.data_ptr()) if isinstance(frames_, torch.Tensor) else frames_,
                                          L.ptr(vrange), L.ptr(ws_), B, n, T_, H_, W_, F, K_, stream)

    assert frames.data_ptr() % 4 == 0
    bad = {
        "null prediction": call(pred_=None),
        "null std": call(std_=None),
        "null workspace with an auto-scaled feature": call(ws_=None),
        "K above the cap": call(K_=handle.p4c_forecast_max_features() + 1),
        "sample == B": call(samples=(0, B)),
        "negative sample": call(samples=(-1, 0)),
        "unaligned frames": call(frames_=ctypes.c_void_p(frames.data_ptr() + 1)),
        "2^31 pixels": call(H_=1 << 15, W_=1 << 15, n=1, K_=2),
    }
    torch.cuda.synchronize()
    assert all(rc == L.ERR_INVALID for rc in bad.values()), bad
    assert handle.p4c_last_error()
    assert bool((frames == 0xA5).all()) and bool((vrange == -777.0).all())
    assert call() == L.OK                                         # the same arguments, none of them bad
    torch.cuda.synchronize()
    assert bool((frames[:B * T * K * H * W] != 0xA5).any()) and bool((frames[B * T * K * H * W:] == 0xA5).all())


def test_wrapper_checks_its_arguments(gpu_device):
    from py4cast_amd import _lib as L

    c = cf.case("b")
    with pytest.raises(L.P4CError, match="feature indices"):
        _run(dict(c, features=(0, 5)), gpu_device)
    with pytest.raises(L.P4CError, match="sample indices"):
        _run(dict(c, samples=(0, 2)), gpu_device)
    with pytest.raises(L.P4CError, match="display rows"):
        _run(dict(c, display=c["display"][:-1]), gpu_device)
    with pytest.raises(L.P4CError, match="finite"):
        _run(dict(c, display=[(None, None, -cf.INF, 1.0)] + c["display"][1:]), gpu_device)


# ------------------------------------------------------------------------------------------------ predict_step and Trainer.predict
TITAN = {"template_grib": "t.grib", "path_to_runtime": "dataset_{}/{}", "output_kwargs": ["titan_1s40"],
         "gif_fmt": "{}_feature_{}.gif", "gif_identifiers": ["runtime", "feature"]}
H1, W1, T1, F1 = 33, 47, 3, 12


def _module(gpu_device, tmp_path):
    """the smallest HalfUNet of tests/test_padded_rollout_gpu.py on its 33 x 47 grid (autopad_enabled), T = 3 from the forcing"""
    from helpers import make_batch, make_dataset_info, synthetic_case
    from py4cast_amd.lightning import AutoRegressiveLightning

    case = synthetic_case(seed=6, B=2, T=T1, T_in=1, H=H1, W=W1, F=F1, Ff=5, Fs=4, border=2)
    info = make_dataset_info(case, case["forcing"].shape[-1])
    torch.manual_seed(0)
    lm = AutoRegressiveLightning(
        dict(autopad_enabled=True), info, None, num_input_steps=1, num_pred_steps_train=T1, batch_size=2, model_name="HalfUNet",
        losses=[{"class": "WeightedLoss", "weight": 0.7, "params": {"loss": "MSELoss", "reduction": "none"}}], training_strategy="scaled_ar",
    ).to(gpu_device)
    lm.train()
    lm.use_native_rollout = True
    lm.training_step(make_batch(case, gpu_device), 0)   # records the names, moves the running statistics
    lm.eval()
    io = tmp_path / "io.json"
    io.write_text(json.dumps(dict(TITAN, dir_grib=str(tmp_path / "gribs"), dir_gif=str(tmp_path / "gifs"))))
    return lm, case, io


def _batch(case, dev, scale=1.0):
    from helpers import GRID_DIMS, feature_names
    from py4cast_amd.base import ItemBatch
    from py4cast_amd.namedtensor import NamedTensor

    return ItemBatch(NamedTensor((case["inputs"] * scale).clone().to(dev), GRID_DIMS, feature_names(F1)),
                     NamedTensor(case["forcing"].clone().to(dev), GRID_DIMS, [f"g{i}" for i in range(5)]), None)


def _check_gifs(root, runtime, returned, b, names, offsets=None):
    """every GIF and sidecar of one sample against the closed form of the RETURNED (un-normalised) prediction: with std 1 and mean 0
    the restatement's v is the returned value itself"""
    from PIL import Image

    from py4cast_amd.outputs import display_for, palette_for

    display = display_for(names, None, offsets)
    rows = [(d.offset if d.offset else None, d.floor, d.vmin, d.vmax) for d in display]
    F = len(names)
    v, bad, vrange = cf.values(returned, torch.ones(F), torch.zeros(F), rows, samples=[b])
    want = cf.indices(v.numpy(), bad.numpy(), vrange.numpy(), H1, W1)
    assert float(want["band"].mean()) <= 1e-2
    files = sorted(p.name for p in (root / "dataset_titan_1s40" / runtime).iterdir())
    assert files == sorted([f"{runtime}_feature_{f}.gif" for f in names] + [f"{runtime}_feature_{f}.gif.json" for f in names])
    for k, f in enumerate(names):
        path = root / "dataset_titan_1s40" / runtime / f"{runtime}_feature_{f}.gif"
        palette = palette_for(display[k].cmap)
        with Image.open(path) as gif:
            assert gif.size == (W1, H1) and gif.info.get("loop") == 0
            total = 0
            for t in range(gif.n_frames):
                gif.seek(t)
                total += gif.info["duration"]
            assert total == 500 * T1                               # (identical neighbours are merged into one longer frame)
            if gif.n_frames == T1:
                for t in range(T1):
                    gif.seek(t)
                    keep = ~want["band"][0, t, k]
                    assert np.array_equal(np.asarray(gif.convert("RGB"))[keep], palette[want["index"][0, t, k]][keep]), (f, t)
            else:
                assert any(np.array_equal(want["index"][0, t, k], want["index"][0, t + 1, k]) for t in range(T1 - 1))
        side = json.loads((path.parent / (path.name + ".json")).read_text())
        assert side["feature"] == f and side["runtime"] == runtime and side["colormap"] == display[k].cmap
        assert side["titles"] == [f"{runtime} +{t + 1}h" for t in range(T1)]
        assert side["ranges"] == [[float(x) for x in vrange[0, t, k]] for t in range(T1)]


def test_predict_step_with_io_conf_writes_the_accepted_samples(gpu_device, tmp_path, monkeypatch):
    from datetime import datetime

    from helpers import feature_names
    from py4cast_amd import _lib as L

    lm, case, io = _module(gpu_device, tmp_path)
    plain = lm.predict_step(_batch(case, gpu_device), 1)
    assert getattr(lm, "forecast_writer", None) is None and not (tmp_path / "gifs").exists()
    dates = [datetime(2023, 1, 1, 0), datetime(2023, 1, 1, 3), datetime(2023, 1, 2, 12), datetime(2023, 1, 2, 6)]
    lm.infer_ds = types.SimpleNamespace(sample_list=[types.SimpleNamespace(timestamps=types.SimpleNamespace(datetime=d)) for d in dates])
    lm.trainer = types.SimpleNamespace(datamodule=types.SimpleNamespace(list_run_hour=[0, 12], save_gifs=True, save_gribs=False))
    lm.io_conf = io
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    out = lm.predict_step(_batch(case, gpu_device), 1)            # samples 2 and 3 of the list: 12 h is a run hour, 6 h is not
    assert calls.count("p4c_forecast_frames") == 1
    lm.forecast_writer.drain()
    assert out.tensor.shape == plain.tensor.shape and torch.equal(_bits(out.tensor), _bits(plain.tensor))
    assert out.names == plain.names and out.feature_names == plain.feature_names
    assert sorted(p.name for p in (tmp_path / "gifs" / "dataset_titan_1s40").iterdir()) == ["2023010212"]
    _check_gifs(tmp_path / "gifs", "2023010212", out.tensor.cpu(), 0, feature_names(F1))
    # a batch without an accepted sample launches nothing and writes nothing
    lm.trainer.datamodule.list_run_hour = [1]
    calls.clear()
    again = lm.predict_step(_batch(case, gpu_device), 1)
    lm.forecast_writer.drain()
    assert calls.count("p4c_forecast_frames") == 0 and torch.equal(_bits(again.tensor), _bits(plain.tensor))
    assert sorted(p.name for p in (tmp_path / "gifs" / "dataset_titan_1s40").iterdir()) == ["2023010212"]


def test_trainer_predict_over_three_batches_with_two_slots(gpu_device, tmp_path):
    """Trainer.predict drains the writer; three batches through two rotating slots give three correct sets of files (the first
    batch's slot is reused by the third), with an offset feature drawn from the module's own writer"""
    from helpers import feature_names
    from py4cast_amd.outputs import ForecastGifWriter, OutputSavingSettings
    from py4cast_amd.trainer import Trainer

    lm, case, io = _module(gpu_device, tmp_path)
    lm.io_conf = io
    offsets = {"f3": -1.5}
    lm.forecast_writer = ForecastGifWriter(OutputSavingSettings.from_json(io), gpu_device, slots=2, offsets=offsets)
    scales = (1.0, 0.5, -1.25)
    preds = Trainer(device=gpu_device).predict(lm, [_batch(case, gpu_device, s) for s in scales])
    assert len(preds) == 3 and not lm.forecast_writer._pending and lm.forecast_writer.slots == 2
    assert not torch.equal(preds[0].tensor, preds[2].tensor)
    names = feature_names(F1)
    runtimes = [f"sample{i:06d}" for i in range(6)]
    assert sorted(p.name for p in (tmp_path / "gifs" / "dataset_titan_1s40").iterdir()) == runtimes
    assert [p.parent.name for p in lm.forecast_writer.written[::F1]] == runtimes          # batch by batch, in order
    for i, runtime in enumerate(runtimes):
        _check_gifs(tmp_path / "gifs", runtime, preds[i // 2].tensor.cpu(), i % 2, names, offsets)
    # the same module without io_conf returns the same bits and writes nothing more
    lm.io_conf = None
    before = len(lm.forecast_writer.written)
    plain = Trainer(device=gpu_device).predict(lm, [_batch(case, gpu_device, scales[2])])
    assert torch.equal(_bits(plain[0].tensor), _bits(preds[2].tensor)) and len(lm.forecast_writer.written) == before
