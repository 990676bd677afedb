"""
ops.grib_pack_complex (csrc/grib_pack_complex.hip) and the complex-packing route of the GRIB writer on the GPU.

``params`` and the payloads are compared BYTE FOR BYTE with bytes that never come from the code under test
(tests/grib_pack_complex_cases.py: the integers of tests/grib2_reference.py's float64 packer through the independent encoder of
tests/grib_complex_cases.py in groups of 32).  Every operation of the contract is exact or a single rounded one and min / max are
order-free, so there is no tolerance and no excluded element.  Unspecified are only words 5 .. 8 of the params of a field that holds a
value that is not finite (``bad`` > 0: its length is 0).  Every byte of the buffer outside the payloads must stay untouched.
tests/test_grib_pack_complex_cpu.py checks the numpy path of py4cast_amd/grib2.py against the same bytes.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib2_reference as ref  # noqa: E402
import grib_complex_cases as cases  # noqa: E402
import grib_pack_complex_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5

#        B  T   H    W   F  samples  features               spec (D, nbits, order) per packed feature                        flip
SHAPES = {
    "gather": (2, 2, 18, 28, 21, None, (0, 3, 7, 8, 15, 20), [(2, 16, 2), (0, 12, 0), (-1, 16, 1), (2, 8, 2), (0, 11, 1), (2, 24, 2)], False),
    "dense": (2, 2, 18, 28, 8, (1,), (0, 1, 2, 4, 5, 7), [(0, 32, 0), (2, 16, 2), (-1, 24, 1), (2, 12, 0), (0, 29, 2), (2, 30, 1)], True),
    "tail_dense": (1, 1, 5, 7, 3, None, (0, 1, 2), [(2, 16, 2), (0, 1, 1), (-1, 12, 0)], True),
    "tail_gather": (1, 2, 5, 7, 8, None, (6, 1), [(0, 11, 2), (2, 24, 1)], False),
    "grid_dense": (1, 1, 37, 53, 3, None, (0, 1, 2), [(2, 16, 2), (0, 12, 1), (-1, 24, 0)], True),
    "grid_gather": (1, 1, 37, 53, 9, None, (8, 1, 4), [(2, 1, 0), (0, 24, 2), (2, 16, 1)], False),
}
for _n in (1, 2, 31, 32, 33):     # the sizes around one group, in both read forms
    SHAPES[f"n{_n:02d}_dense"] = (1, 1, 1, _n, 3, None, (0, 1, 2), [(2, 16, 0), (0, 12, 1), (-1, 24, 2)], False)
    SHAPES[f"n{_n:02d}_gather"] = (1, 1, 1, _n, 8, None, (5, 0, 3), [(2, 29, 2), (0, 32, 0), (-1, 30, 1)], False)


def _tensors(c, dev):
    return (torch.from_numpy(c["pred"]).to(dev), torch.from_numpy(c["std"]).to(dev), torch.from_numpy(c["mean"]).to(dev))


def _run(c, dev):
    """-> (params, buffer of the capacity) numpy; the call writes into the middle of two sentinel-filled buffers, is repeated, and
    both must agree"""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    B, T, H, W, F = c["pred"].shape
    n, K = len(c["samples"]), len(c["features"])
    capacity = ops.grib_complex_capacity(n, T, H * W, c["spec"])
    assert capacity == n * T * sum(pc.capacity(H * W, nbits, order) for _, nbits, order in c["spec"])
    host_spec = (ctypes.c_int32 * (3 * K))(*[x for triple in c["spec"] for x in triple])
    assert L.lib().p4c_grib_pack_complex_capacity(n, T, H * W, host_spec, K) == capacity
    pbytes = n * T * K * ops.GRIB_COMPLEX_PARAMS * 4
    outs = []
    for _ in range(2):
        pbuf = torch.full((GUARD + pbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
        sbuf = torch.full((GUARD + capacity + GUARD,), FILL, dtype=torch.uint8, device=dev)
        out = (pbuf[GUARD:GUARD + pbytes].view(torch.int32).view(n, T, K, ops.GRIB_COMPLEX_PARAMS), sbuf[GUARD:GUARD + capacity])
        got = ops.grib_pack_complex(*_tensors(c, dev), c["spec"], samples=c["samples"], features=c["features"], flip_rows=c["flip"], out=out)
        assert got[0] is out[0] and got[1] is out[1]
        torch.cuda.synchronize()
        for buf, size in ((pbuf, pbytes), (sbuf, capacity)):
            assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + size:] == FILL).all()), "a sentinel was overwritten"
        outs.append((out[0].cpu().numpy(), out[1].cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), "two calls differ"
    return outs[0]


def _expected(c):
    B, T, h, w, F = c["pred"].shape
    return pc.expected_call(c["pred"].reshape(B, T, h * w, F), c["std"], c["mean"], c["spec"], c["samples"], c["features"], h, w, c["flip"])


def _check(c, dev, expected=None):
    """params, every payload and every byte outside the payloads; -> (params, buffer, payloads, integers)"""
    params, payloads, ints = _expected(c) if expected is None else expected
    got, buf = _run(c, dev)
    assert got.shape == params.shape
    bad = params[..., 4] > 0
    assert np.array_equal(got[~bad], params[~bad]), "params differ from the independent encoder's numbers"
    assert np.array_equal(got[bad][:, [0, 1, 2, 3, 4, 9, 10]], params[bad][:, [0, 1, 2, 3, 4, 9, 10]])
    written = np.zeros(buf.size, dtype=bool)
    for (i, t, k), payload in payloads.items():
        at = int(params[i, t, k, 10])
        assert at % 4 == 0 and buf[at:at + len(payload)].tobytes() == payload, (i, t, k)
        written[at:at + len(payload)] = True
    assert (buf[~written] == FILL).all(), "a byte outside the payloads was written"
    return got, buf, payloads, ints


@pytest.fixture(scope="module")
def forms():
    from py4cast_amd import _lib as L

    return lambda K, F: bool(L.lib().p4c_grib_pack_dense(K, F))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_params_and_payloads_byte_for_byte(name, gpu_device, forms):
    """gather / dense: the data cases of the simple packer's test with an order per feature: one call mixes orders 0, 1, 2 and widths
    8 .. 32, K is gathered from a wider F, rows flipped in the dense case, W = 28 (groups straddle rows), a constant field and a field
    with one NaN (bad > 0, length 0, the neighbours unmoved: their offsets are the expected ones); tail_*: 35 points; grid_*: 37 x 53;
    nXX_*: 1, 2, 31, 32, 33 points, with the widest nbits of every order"""
    B, T, H, W, F, samples, features, spec, flip = SHAPES[name]
    assert forms(len(features), F) == ("dense" in name)
    c = ref.case(SHAPES[name])
    got, buf, payloads, ints = _check(c, gpu_device)
    if len(features) > 3:
        bad = got[..., 4]
        assert bad.sum() == 1 and bad[len(c["samples"]) - 1, 0, 2] == 1 and got[len(c["samples"]) - 1, 0, 2, 9] == 0
        const = got[0, T - 1, 3]
        order = spec[3][2]
        ng = -(-H * W // 32)
        assert const[0] == const[1] and const[8] == 0 and const[9] == (4 * (order + 1) if order else 0) + (6 * ng + 7) // 8
    assert H * W <= 5000                                       # the sequential decoder reads the integers back
    for (i, t, k), payload in payloads.items():
        if ints[i, t, k] is not None:
            D, nbits, order = spec[k]
            R, E = float(got[i, t, k, 2:3].view(np.float32)[0]), int(got[i, t, k, 3])
            numbers = dict(order=order, nbytes=4 if order else 0, ng=-(-H * W // 32), ref_bits=int(got[i, t, k, 8]), w_ref=0, w_bits=6, l_ref=32,
                           l_inc=1, l_last=H * W - 32 * (-(-H * W // 32) - 1), l_bits=0)
            at = int(got[i, t, k, 10])
            msg = cases.assemble(W, H, cases.section5(H * W, R, E, D, numbers), buf[at:at + int(got[i, t, k, 9])].tobytes())
            assert cases.restate(msg)[0] == ints[i, t, k], (i, t, k)


def test_the_orders_widths_and_forms_are_all_covered():
    specs = [s for shape in SHAPES.values() for s in shape[7]]
    assert {o for _, _, o in specs} == {0, 1, 2} and {1, 12, 16, 24} <= {b for _, b, _ in specs}
    assert {(pc.LIMITS[o], o) for o in (0, 1, 2)} <= {(b, o) for _, b, o in specs}
    assert {s[8] for s in SHAPES.values()} == {True, False} and any(s[3] % 32 and s[2] > 1 for s in SHAPES.values())


# B, T, H, W, F, samples, features, spec, flip: n*T = 512 pairs leave two workgroups per pair
LOOP = {"dense": (32, 16, 12, 25, 2, None, (1,), [(2, 16, 2)], True),
        "gather": (32, 16, 12, 25, 3, None, (2,), [(0, 11, 1)], False)}


@pytest.mark.parametrize("form", ["dense", "gather"])
def test_past_one_loop_trip_of_the_tile_and_offset_launches(form, gpu_device, forms):
    """the smallest grid that sends a workgroup of the range, group and pack launches through a second trip with every field spread
    over two workgroups, from the library's own launch arithmetic; more fields than one trip of the offsets launch takes"""
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    handle = L.lib()
    tile, cap = handle.p4c_grib_tile(), handle.p4c_grib_max_blocks()
    assert (tile, cap) == (ops.GRIB_TILE, ops.GRIB_MAX_BLOCKS)
    assert (handle.p4c_grib_pack_complex_group(), handle.p4c_grib_pack_complex_params(), handle.p4c_grib_pack_complex_scan_threads()) == (
        ops.GRIB_COMPLEX_GROUP, ops.GRIB_COMPLEX_PARAMS, ops.GRIB_COMPLEX_SCAN_THREADS)
    B, T, H, W, F, _, features, spec, flip = LOOP[form]
    per_pair = cap // (B * T)
    N = H * W
    tiles = -(-N // tile)
    assert per_pair == 2 and per_pair < tiles <= 2 * per_pair and N % tile and N % 32 and N % 8
    assert B * T * len(features) > ops.GRIB_COMPLEX_SCAN_THREADS and B * T * N * len(features) <= 200_000
    assert forms(len(features), F) == (form == "dense")
    _check(ref.case(LOOP[form]), gpu_device)


def test_past_one_loop_trip_of_the_scan_and_table_launches(gpu_device):
    """one field of more groups than a workgroup of the scan launch takes in a trip, and of more than 8 times as many: a second trip of
    the tables launch; the carry of the scan crosses trips"""
    from py4cast_amd import ops

    shape = (1, 1, 2, 32788, 1, None, (0,), [(2, 12, 2)], False)
    N = shape[2] * shape[3]
    assert -(-N // 32) > 8 * ops.GRIB_COMPLEX_SCAN_THREADS and N % 32 and N <= 200_000
    g = np.random.default_rng(8)
    c = ref.case(shape)
    x = np.arange(N, dtype=np.float64)
    c["pred"] = (np.sin(x / 400.0) + 0.01 * (x / N) * g.standard_normal(N)).astype(np.float32).reshape(c["pred"].shape)
    _check(c, gpu_device)


@pytest.mark.parametrize("form", ["dense", "gather"])
def test_the_differences_across_every_tile_and_workgroup_boundary(form, gpu_device, forms):
    """a staircase with a jump at every tile boundary, one point before it and one point after it (a feature each), at orders 1 and 2:
    each tile is another workgroup's, so the two points before a tile come from global memory"""
    from py4cast_amd import ops

    tile = ops.GRIB_TILE
    H, W = 1, 5 * tile + 17
    F = 6 if form == "dense" else 13
    features = tuple(range(6)) if form == "dense" else (12, 1, 3, 5, 8, 10)
    spec = [(0, 12, 1), (0, 12, 1), (0, 12, 1), (0, 12, 2), (0, 12, 2), (0, 12, 2)]
    assert forms(len(features), F) == (form == "dense") and ops.GRIB_MAX_BLOCKS // 2 >= -(-W // tile)
    c = ref.case((1, 2, H, W, F, None, features, spec, False))
    q = np.arange(W)
    g = np.random.default_rng(2)
    for k, f in enumerate(features):
        shift = (-1, 0, 1)[k % 3]
        steps = ((q - shift) // tile).astype(np.float32)           # the jump sits at boundary + shift
        for t in range(2):
            c["pred"][0, t, 0, :, f] = steps * (1.0 if t == 0 else -1.5) + 0.01 * g.standard_normal(W).astype(np.float32)
    got, buf, payloads, ints = _check(c, gpu_device)
    for (i, t, k), X in ints.items():
        jumps = [abs(X[b + (-1, 0, 1)[k % 3]] - X[b + (-1, 0, 1)[k % 3] - 1]) for b in range(tile, W, tile)]
        assert min(jumps) > 20 * 4                                   # the jump is there, far above the noise


def test_a_strided_view_of_a_larger_buffer(gpu_device):
    """the native rollout hands over ``states[:, T_in:]``: a batch stride larger than T*N*F"""
    from py4cast_amd import ops

    c = ref.case(SHAPES["dense"])
    params, payloads, _ = _expected(c)
    B, T, H, W, F = c["pred"].shape
    big = torch.full((B, T + 2, H, W, F), 7.0, device=gpu_device)
    big[:, 2:] = torch.from_numpy(c["pred"]).to(gpu_device)
    view = big[:, 2:]
    assert not view.is_contiguous()
    got, stream = ops.grib_pack_complex(view, *_tensors(c, gpu_device)[1:], c["spec"], samples=c["samples"], features=c["features"],
                                        flip_rows=c["flip"])
    got, stream = got.cpu().numpy(), stream.cpu().numpy()
    bad = params[..., 4] > 0
    assert np.array_equal(got[~bad], params[~bad])
    for (i, t, k), payload in payloads.items():
        at = int(params[i, t, k, 10])
        assert stream[at:at + len(payload)].tobytes() == payload


def test_bad_arguments_return_the_code_and_launch_nothing(gpu_device):
    from py4cast_amd import _lib as L

    handle = L.lib()
    B, T, H, W, F, K = 2, 1, 4, 8, 3, 3
    dev = gpu_device
    pred = torch.randn(B, T, H, W, F, device=dev)
    std, mean = torch.ones(F, device=dev), torch.zeros(F, device=dev)
    feats = torch.arange(K, dtype=torch.int32, device=dev)
    good = ((2, 16, 2), (0, 12, 0), (0, 8, 1))
    capacity = B * T * sum(pc.capacity(H * W, nbits, order) for _, nbits, order in good)
    out = torch.full((capacity + 8,), FILL, dtype=torch.uint8, device=dev)
    params = torch.full((B, T, K, 11), -777, dtype=torch.int32, device=dev)
    ws = torch.empty(handle.p4c_grib_pack_complex_workspace_bytes(B, T, H * W, K, F) // 8 + 2, dtype=torch.int64, device=dev)
    stream = L.stream(dev)

    def call(pred_=pred, samples=(0, 1), std_=std, out_=out, ws_=ws, n=B, K_=K, H_=H, W_=W, spec=good, bytes_=capacity, host=True):
        host_samples = (ctypes.c_int32 * len(samples))(*samples) if host else None
        host_spec = (ctypes.c_int32 * (3 * len(spec)))(*[x for triple in spec for x in triple]) if spec is not None else None
        return handle.p4c_grib_pack_complex(L.ptr(pred_), T * H * W * F, H * W * F, host_samples, L.ptr(std_), L.ptr(mean), L.ptr(feats),
                                            host_spec, 0, L.ptr(params),
                                            ctypes.c_void_p(out_.data_ptr()) if isinstance(out_, torch.Tensor) else out_, bytes_,
                                            L.ptr(ws_), B, n, T, H_, W_, F, K_, stream)

    assert out.data_ptr() % 4 == 0 and ws.data_ptr() % 16 == 0
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
        "nbits 0": call(spec=((2, 16, 0), (0, 0, 0), (0, 8, 0))),
        "nbits 33": call(spec=((2, 16, 0), (0, 33, 0), (0, 8, 0))),
        "D 16": call(spec=((16, 16, 0), (0, 8, 0), (0, 8, 0))),
        "D -16": call(spec=((-16, 16, 0), (0, 8, 0), (0, 8, 0))),
        "order 3": call(spec=((2, 16, 3), (0, 8, 0), (0, 8, 0)), bytes_=1 << 20),
        "order -1": call(spec=((2, 16, -1), (0, 8, 0), (0, 8, 0)), bytes_=1 << 20),
        "nbits 31 at order 1": call(spec=((2, 31, 1), (0, 8, 0), (0, 8, 0)), bytes_=1 << 20),
        "nbits 30 at order 2": call(spec=((2, 30, 2), (0, 8, 0), (0, 8, 0)), bytes_=1 << 20),
        "unaligned out": call(out_=ctypes.c_void_p(out.data_ptr() + 1)),
        "a buffer below the capacity": call(bytes_=capacity - 1),
        "2^31 payload bytes": call(H_=1 << 15, W_=1 << 14, n=1, K_=1, spec=((0, 32, 0),), bytes_=1 << 40),
        "2^31 grid points": call(H_=1 << 16, W_=1 << 15, n=1, K_=1, spec=((0, 1, 0),), bytes_=1 << 40),
    }
    torch.cuda.synchronize()
    assert all(rc == L.ERR_INVALID for rc in bad.values()), bad
    assert handle.p4c_last_error()
    assert bool((out == FILL).all()) and bool((params == -777).all())
    host_spec = (ctypes.c_int32 * 9)(*[x for triple in ((2, 31, 1), (0, 8, 0), (0, 8, 0)) for x in triple])
    assert handle.p4c_grib_pack_complex_capacity(B, T, H * W, host_spec, K) == -1
    assert call() == L.OK                                         # the same arguments, none of them bad
    torch.cuda.synchronize()
    assert bool((out[:capacity] != FILL).any()) and bool((out[capacity:] == FILL).all())
    assert bool((params != -777).all())


def test_wrapper_checks_its_arguments(gpu_device):
    from py4cast_amd import _lib as L
    from py4cast_amd import ops

    c = ref.case(SHAPES["tail_gather"])
    dev = gpu_device
    pred, std, mean = _tensors(c, dev)
    with pytest.raises(L.P4CError, match="feature indices"):
        ops.grib_pack_complex(pred, std, mean, c["spec"], features=(0, 8))
    with pytest.raises(L.P4CError, match="triples for"):
        ops.grib_pack_complex(pred, std, mean, c["spec"][:1], features=c["features"])
    for spec in ([(0, 40, 0), (0, 8, 0)], [(0, 31, 1), (0, 8, 0)], [(0, 30, 2), (0, 8, 0)], [(0, 8, 3), (0, 8, 0)]):
        with pytest.raises(L.P4CError, match="nbits"):
            ops.grib_pack_complex(pred, std, mean, spec, features=c["features"])
    with pytest.raises(L.P4CError, match="out:"):
        ops.grib_pack_complex(pred, std, mean, c["spec"], features=c["features"],
                              out=(torch.empty(1, 2, 2, 11, dtype=torch.int32, device=dev), torch.empty(8, dtype=torch.uint8, device=dev)))
    with pytest.raises(L.P4CError, match="GPU only"):
        ops.grib_pack_complex(pred.cpu(), std, mean, c["spec"], features=c["features"])


@pytest.mark.parametrize("name", ["gather", "dense", "grid_dense"])
def test_the_device_decoder_reads_the_planes_of_the_simple_route(name, gpu_device):
    """ops.grib_pack_complex -> ops.grib_unpack_complex equals ops.grib_pack -> ops.grib_unpack for the same prediction, bit for bit"""
    from py4cast_amd import ops

    B, T, H, W, F, samples, features, spec, flip = SHAPES[name]
    c = ref.case(SHAPES[name])
    c["pred"] = np.nan_to_num(c["pred"], nan=0.25)                  # every field is written
    dev = gpu_device
    n, K, N = len(c["samples"]), len(features), H * W
    cp, stream = ops.grib_pack_complex(*_tensors(c, dev), spec, samples=c["samples"], features=features, flip_rows=flip)
    simple = [(D, nbits) for D, nbits, _ in spec]
    sp, packed = ops.grib_pack(*_tensors(c, dev), simple, samples=c["samples"], features=features, flip_rows=flip)
    cp_h, sp_h, pitch = cp.cpu().numpy().reshape(-1, 11), sp.cpu().numpy().reshape(-1, 5), packed.shape[-1]
    assert np.array_equal(cp_h[:, :5], sp_h) and not cp_h[:, 4].any()
    ng = -(-N // 32)
    complex_fields, simple_fields = [], []
    for i in range(n * T * K):
        D, nbits, order = spec[i % K]
        R = float(cp_h[i, 2:3].view(np.float32)[0])
        complex_fields.append(dict(stream_off=int(cp_h[i, 10]), stream_len=int(cp_h[i, 9]), ni=W, nj=H, count=N, ng=ng, ref_bits=int(cp_h[i, 8]),
                                   w_ref=0, w_bits=6, l_ref=32, l_inc=1, l_last=N - 32 * (ng - 1), l_bits=0, order=order, nbytes=4 if order else 0,
                                   ival1=int(cp_h[i, 5]), ival2=int(cp_h[i, 6]), gmin=int(cp_h[i, 7]), E=int(cp_h[i, 3]), D=D, R=R))
        simple_fields.append(dict(stream_off=i * pitch, stream_len=(N * nbits + 7) // 8, ni=W, nj=H, count=N, nbits=nbits, E=int(sp_h[i, 3]), D=D, R=R))
    a, status = ops.grib_unpack_complex(stream, complex_fields)
    b = ops.grib_unpack(packed.reshape(-1), simple_fields)
    torch.cuda.synchronize()
    assert not bool(status.any())
    pad = (N + 3) // 4 * 4                                          # a plane starts at a multiple of 4 floats
    a, b = a.view(torch.int32).view(n * T * K, pad)[:, :N], b.view(torch.int32).view(n * T * K, pad)[:, :N]
    assert torch.equal(a, b)


def _mixed_template(south_to_north=False):
    """ref.template_file with message 1 (u10) re-packed in 5.2, message 3 (r2) in 5.3 at order 1 and message 4 (pmer) in 5.3 at order 2
    by the independent encoder; the others stay in 5.0"""
    import struct

    out = []
    data = ref.template_file(south_to_north=south_to_north)
    at = 0
    for i, sections in enumerate(ref.walk(data)):
        total = struct.unpack_from(">Q", sections[0], 8)[0]
        msg = data[at:at + total]
        at += total
        order = {1: 0, 3: 1, 4: 2}.get(i)
        if order is not None:
            k = ref.keys(sections)
            X = pc.integers(sections[7][5:], k["count"], k["nbits"])
            numbers, payload, _ = cases.encode(X, order, range(0, len(X), 40), nbytes=4 if order else 0, ref_bits=k["nbits"])
            msg = cases.patched(msg, 5, lambda s, n=numbers, k=k: bytearray(cases.section5(k["count"], k["R"], k["E"], k["D"], n)))
            msg = cases.patched(msg, 7, lambda s, p=payload: bytearray(s[:5]) + p)
        out.append(msg)
    return b"".join(out)


@pytest.mark.parametrize("packing", ["template", "complex"])
def test_the_device_writer_writes_the_cpu_writers_bytes(packing, gpu_device, tmp_path):
    """the same prediction through ForecastGribWriter on the device and on the CPU: identical files, over two batches (two slots);
    "template" over a template with 5.0, 5.2 and 5.3 messages makes the simple and the complex call in one submit"""
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
        (root / "template.grib").write_bytes(_mixed_template())
        io = root / "io.json"
        io.write_text(json.dumps({"template_grib": "../template.grib", "path_to_runtime": "{}", "dir_grib": str(root / "gribs"),
                                  "dir_gif": str(root / "gifs"), "grib_fmt": "mb{}_ech_{}.grib", "grib_identifiers": ["member", "leadtime"]}))
        writer = ForecastGribWriter(OutputSavingSettings.from_json(io), device, lat, lon, packing=packing)
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
    want = [0, 2, 3, 0, 3] if packing == "template" else [3] * 5       # t2m, u10, pmer, tp, r2 in the prediction's order
    for name, data in files["cpu"].items():
        assert files["gpu"][name] == data, name
        messages = grib2.parse_messages(data)
        assert [m.keys["dataRepresentationTemplateNumber"] for m in messages] == want


@pytest.mark.parametrize("name", ["gather", "dense", "tail_dense"])
def test_both_forms_of_the_pack_pass_write_the_expected_bytes(name, gpu_device, diag_library, monkeypatch):
    """the A/B switch of the diagnostic library (profiles/grib_pack_complex.txt): the pack pass reads differences that the group pass
    stored, or the prediction again -- the same bytes either way"""
    c = ref.case(SHAPES[name])
    expected = _expected(c)
    for flag in ("1", "0"):
        monkeypatch.setenv("P4C_GRIB_CPX_STORED", flag)
        _check(c, gpu_device, expected)
