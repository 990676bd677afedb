"""
ops.grib_pack (csrc/grib_pack.hip) and the GRIB writer on the GPU.

``params`` and the bit streams are compared BYTE FOR BYTE with the float64 restatement of tests/grib2_reference.py: every operation of
the contract is a single rounded one and min / max are order-free, so there is no tolerance and no excluded element.  The only
unspecified bytes are the stream of a field that holds a value that is not finite (it is reported through ``bad``) and the padding of
a row of ``packed`` past its stream, which must stay untouched.  tests/test_grib2_cpu.py checks the restatement against the numpy
path of py4cast_amd/grib2.py on the same inputs.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib2_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5


def _run(c, dev):
    """-> (params, packed) numpy; the call writes into the middle of two sentinel-filled buffers, is repeated, and both must agree"""
    from py4cast_amd import ops

    B, T, H, W, F = c["pred"].shape
    n, K = len(c["samples"]), len(c["features"])
    pitch = ops.grib_pitch(H * W, c["spec"])
    pbytes, sbytes = n * T * K * ops.GRIB_PARAMS * 4, n * T * K * pitch
    outs = []
    for _ in range(2):
        pbuf = torch.full((GUARD + pbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
        sbuf = torch.full((GUARD + sbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
        out = (pbuf[GUARD:GUARD + pbytes].view(torch.int32).view(n, T, K, ops.GRIB_PARAMS), sbuf[GUARD:GUARD + sbytes].view(n, T, K, pitch))
        got = ops.grib_pack(torch.from_numpy(c["pred"]).to(dev), torch.from_numpy(c["std"]).to(dev), torch.from_numpy(c["mean"]).to(dev),
                            c["spec"], samples=c["samples"], features=c["features"], flip_rows=c["flip"], out=out)
        assert got[0] is out[0] and got[1] is out[1]
        torch.cuda.synchronize()
        for buf, size in ((pbuf, pbytes), (sbuf, sbytes)):
            assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + size:] == FILL).all()), "a sentinel was overwritten"
        outs.append((out[0].cpu().numpy(), out[1].cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), "two calls differ"
    return outs[0]


def _check(c, dev):
    params, streams = ref.expected_of(c)
    got, packed = _run(c, dev)
    assert got.shape == params.shape and np.array_equal(got, params), "params differ from the float64 restatement"
    compared = 0
    for (i, t, k), stream in streams.items():
        if stream is None:
            continue
        assert packed[i, t, k, :len(stream)].tobytes() == stream, (i, t, k)
        assert (packed[i, t, k, len(stream):] == FILL).all(), "the padding of a row was written"
        compared += 1
    return got, packed, streams, compared


@pytest.fixture(scope="module")
def forms():
    from py4cast_amd import _lib as L

    return lambda K, F: bool(L.lib().p4c_grib_pack_dense(K, F))


@pytest.mark.parametrize("name", sorted(ref.SHAPES))
def test_params_and_streams_byte_for_byte(name, gpu_device, forms):
    """gather: 6 of 21 features, all samples; dense: 6 of 8, a sub-list of samples, rows flipped; tail_*: 35 points, no multiple of 8.
    Widths 8, 11, 12, 16, 24, 32 and D of 0, 2, -1 between them; a constant field and a field with one NaN in the first two."""
    B, T, H, W, F, samples, features, spec, flip = ref.SHAPES[name]
    assert forms(len(features), F) == ("dense" in name)
    c = ref.case(ref.SHAPES[name])
    got, packed, streams, compared = _check(c, gpu_device)
    if len(features) > 3:
        assert compared == len(streams) - 1
        bad = got[..., 4]
        assert bad.sum() == 1 and bad[len(c["samples"]) - 1, 0, 2] == 1          # the NaN is reported where it is, and nowhere else
        const = got[0, T - 1, 3]
        stream = streams[0, T - 1, 3]
        assert const[0] == const[1] and const[3] == 0 and not any(stream)      # a constant field: E = 0, zeros at the template's width
    else:
        assert compared == len(streams) and (H * W) % 8


def test_the_widths_and_scale_factors_are_all_covered():
    widths = {nbits for s in ref.SHAPES.values() for _, nbits in s[7]}
    assert {8, 11, 12, 16, 24, 32} <= widths and {0, 2, -1} <= {D for s in ref.SHAPES.values() for D, _ in s[7]}
    assert {s[8] for s in ref.SHAPES.values()} == {True, False}


@pytest.mark.parametrize("form", ["dense", "gather"])
def test_past_one_loop_trip_of_every_launch(form, gpu_device, forms):
    """the smallest grid that sends a workgroup of the range launch and of the pack launch through a second trip, from the library's
    own launch arithmetic; the finish launch reads more than one partial per field"""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    handle = L.lib()
    tile, cap = handle.p4c_grib_tile(), handle.p4c_grib_max_blocks()
    assert (tile, cap, handle.p4c_grib_max_features(), handle.p4c_grib_max_samples()) == (
        ops.GRIB_TILE, ops.GRIB_MAX_BLOCKS, ops.GRIB_MAX_FEATURES, ops.GRIB_MAX_SAMPLES)
    B, T, H, W, F, _, features, spec, flip = ref.LOOP[form]
    per_pair = cap // (B * T)
    N = H * W
    tiles = -(-N // tile)
    assert per_pair < tiles <= 2 * per_pair and N % tile and N % 8          # a second trip for some, a ragged last tile, a ragged octet group
    assert handle.p4c_grib_pack_workspace_bytes(B, T, N, len(features)) == B * T * per_pair * len(features) * 3 * 4
    assert forms(len(features), F) == (form == "dense")
    _, _, streams, compared = _check(ref.case(ref.LOOP[form]), gpu_device)
    assert compared == len(streams)


def test_a_strided_view_of_a_larger_buffer(gpu_device):
    """the native rollout hands over ``states[:, T_in:]``: a batch stride larger than T*N*F"""
    from py4cast_amd import ops

    c = ref.case(ref.SHAPES["dense"])
    params, streams = ref.expected_of(c)
    B, T, H, W, F = c["pred"].shape
    big = torch.full((B, T + 2, H, W, F), 7.0, device=gpu_device)
    big[:, 2:] = torch.from_numpy(c["pred"]).to(gpu_device)
    view = big[:, 2:]
    assert not view.is_contiguous()
    got, packed = ops.grib_pack(view, torch.from_numpy(c["std"]).to(gpu_device), torch.from_numpy(c["mean"]).to(gpu_device), c["spec"],
                                samples=c["samples"], features=c["features"], flip_rows=c["flip"])
    assert np.array_equal(got.cpu().numpy(), params)
    packed = packed.cpu().numpy()
    for (i, t, k), stream in streams.items():
        if stream is not None:
            assert packed[i, t, k, :len(stream)].tobytes() == stream


def test_bad_arguments_return_the_code_and_launch_nothing(gpu_device):
    from py4cast_amd import _lib as L

    handle = L.lib()
    B, T, H, W, F, K = 2, 1, 4, 8, 3, 3
    dev = gpu_device
    pred = torch.randn(B, T, H, W, F, device=dev)
    std, mean = torch.ones(F, device=dev), torch.zeros(F, device=dev)
    feats = torch.arange(K, dtype=torch.int32, device=dev)
    pitch = H * W * 2
    packed = torch.full((B * T * K * pitch + 8,), FILL, dtype=torch.uint8, device=dev)
    params = torch.full((B, T, K, 5), -777, dtype=torch.int32, device=dev)
    ws = torch.empty(handle.p4c_grib_pack_workspace_bytes(B, T, H * W, K) // 4 + 1, device=dev)
    stream = L.stream(dev)

    def call(pred_=pred, samples=(0, 1), std_=std, packed_=packed, ws_=ws, n=B, K_=K, H_=H, W_=W, spec=((2, 16),) * K, pitch_=pitch, host=True):
        host_samples = (ctypes.c_int32 * len(samples))(*samples) if host else None
        host_spec = (ctypes.c_int32 * (2 * len(spec)))(*[x for pair in spec for x in pair]) if spec is not None else None
        return handle.p4c_grib_pack(L.ptr(pred_), T * H * W * F, H * W * F, host_samples, L.ptr(std_), L.ptr(mean), L.ptr(feats), host_spec, 0,
                                    L.ptr(params), ctypes.c_void_p(packed_.data_ptr()) if isinstance(packed_, torch.Tensor) else packed_,
                                    pitch_, L.ptr(ws_), B, n, T, H_, W_, F, K_, stream)

    assert packed.data_ptr() % 4 == 0
    bad = {
        "null prediction": call(pred_=None),
        "null std": call(std_=None),
        "null workspace": call(ws_=None),
        "null samples": call(host=False),
        "null spec": call(spec=None),
        "K above the cap": call(K_=handle.p4c_grib_max_features() + 1),
        "n above the cap": call(n=handle.p4c_grib_max_samples() + 1),
        "sample == B": call(samples=(0, B)),
        "negative sample": call(samples=(-1, 0)),
        "nbits 0": call(spec=((2, 16), (0, 0), (0, 8))),
        "nbits 33": call(spec=((2, 16), (0, 33), (0, 8))),
        "D 16": call(spec=((16, 16), (0, 8), (0, 8))),
        "D -16": call(spec=((-16, 16), (0, 8), (0, 8))),
        "unaligned packed": call(packed_=ctypes.c_void_p(packed.data_ptr() + 1)),
        "a pitch that is no multiple of 4": call(pitch_=pitch + 2),
        "a pitch shorter than the stream": call(pitch_=pitch - 4),
        "2^31 stream bytes": call(H_=1 << 15, W_=1 << 14, n=1, K_=2, spec=((0, 16),) * 2, pitch_=1 << 30),
        "2^31 grid points": call(H_=1 << 16, W_=1 << 15, n=1, K_=1, spec=((0, 1),), pitch_=1 << 28),
    }
    torch.cuda.synchronize()
    assert all(rc == L.ERR_INVALID for rc in bad.values()), bad
    assert handle.p4c_last_error()
    assert bool((packed == FILL).all()) and bool((params == -777).all())
    assert call() == L.OK                                         # the same arguments, none of them bad
    torch.cuda.synchronize()
    assert bool((packed[:B * T * K * pitch] != FILL).any()) and bool((packed[B * T * K * pitch:] == FILL).all())
    assert bool((params != -777).any())


def test_wrapper_checks_its_arguments(gpu_device):
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    c = ref.case(ref.SHAPES["tail_gather"])
    dev = gpu_device
    pred, std, mean = (torch.from_numpy(c[k]).to(dev) for k in ("pred", "std", "mean"))
    with pytest.raises(L.P4CError, match="feature indices"):
        ops.grib_pack(pred, std, mean, c["spec"], features=(0, 8))
    with pytest.raises(L.P4CError, match="sample indices"):
        ops.grib_pack(pred, std, mean, c["spec"], samples=(0, 1), features=c["features"])
    with pytest.raises(L.P4CError, match="pairs for"):
        ops.grib_pack(pred, std, mean, c["spec"][:1], features=c["features"])
    with pytest.raises(L.P4CError, match="nbits"):
        ops.grib_pack(pred, std, mean, [(0, 40), (0, 8)], features=c["features"])
    with pytest.raises(L.P4CError, match="GPU only"):
        ops.grib_pack(pred.cpu(), std, mean, c["spec"], features=c["features"])


def test_the_device_writer_writes_the_cpu_writers_bytes(gpu_device, tmp_path):
    """the same prediction through ForecastGribWriter on the device and on the CPU: identical files, over two batches (two slots)"""
    import datetime as dt
    import json
    import types

    from py4cast_amd import grib2
    from py4cast_amd.namedtensor import NamedTensor
    from py4cast_amd.outputs import ForecastGribWriter, GribSample, OutputSavingSettings

    names = ["aro_t2m_2m", "aro_u10_10m", "aro_z_500hpa", "aro_prmsl_0hpa", "aro_tp_0m", "aro_r2_2m"]
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(2, 2, ref.H, ref.W, len(names), generator=g)
    std = torch.tensor([6.0, 4.0, 80.0, 900.0, 1.5, 20.0])
    mean = torch.tensor([283.0, -1.0, 5500.0, 101300.0, 2.0, 60.0])
    lat, lon = ref.forecast_grid()
    files = {}
    for where, device in (("cpu", torch.device("cpu")), ("gpu", gpu_device)):
        root = tmp_path / where
        (root / "gribs").mkdir(parents=True)
        (root / "template.grib").write_bytes(ref.template_file(south_to_north=False))
        io = root / "io.json"
        io.write_text(json.dumps({"template_grib": "../template.grib", "path_to_runtime": "{}", "dir_grib": str(root / "gribs"),
                                  "dir_gif": str(root / "gifs"), "grib_fmt": "mb{}_ech_{}.grib", "grib_identifiers": ["member", "leadtime"]}))
        writer = ForecastGribWriter(OutputSavingSettings.from_json(io), device, lat, lon)
        for batch, scale in enumerate((1.0, -0.5)):
            samples = []
            for b in range(2):
                start = dt.datetime(2023, 1, 1 + batch, 6 * b)
                deltas = [dt.timedelta(hours=i - 1) for i in range(4)]
                sample = types.SimpleNamespace(timestamps=types.SimpleNamespace(datetime=start, timedeltas=deltas), member=b,
                                               output_timestamps=types.SimpleNamespace(datetime=start, timedeltas=deltas[2:]))
                samples.append(GribSample.from_sample(sample, start.strftime("%Y%m%d%H")))
            preds = NamedTensor((pred * scale).to(device), ["batch", "timestep", "lat", "lon", "features"], list(names))
            writer.submit(preds, std.to(device), mean.to(device), samples)
        writer.drain()
        assert len(writer.written) == 8 and not writer._pending
        files[where] = {str(p.relative_to(root)): p.read_bytes() for p in writer.written}
    assert sorted(files["cpu"]) == sorted(files["gpu"]) and len(files["cpu"]) == 8
    for name, data in files["cpu"].items():
        assert files["gpu"][name] == data, name
        assert len(grib2.parse_messages(data)) == 5
