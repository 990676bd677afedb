"""
What the tests of the complex-packing WRITER share (test infrastructure, never product code; not collected).  Expected bytes never come
from the code under test: the integers X come from ``grib2_reference.pack`` (the float64 packer restated with exact rationals), the
payload from ``grib_complex_cases.encode`` (written from the WMO layout) with groups of 32 values, and messages are read back with
``grib_complex_cases.restate``.  The differencing below is restated once more in plain Python integers, only to tell the encoder how
many bits the largest group reference needs (its ``ref_bits`` argument); the encoder asserts that the number fits.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib2_reference as ref  # noqa: E402
import grib_complex_cases as cases  # noqa: E402

GROUP = 32
PARAMS = 11
LIMITS = {0: 32, 1: 30, 2: 29}        # the widest nbits of an order


def integers(stream, count, nbits):
    """the ``count`` integers of a simple-packed stream, as Python integers"""
    bits = np.unpackbits(np.frombuffer(stream, dtype=np.uint8), count=count * nbits).reshape(count, nbits).astype(np.uint64)
    return [int(x) for x in (bits << np.arange(nbits - 1, -1, -1, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)]


def reference_bits(X, order):
    """the bit length of the largest group minimum of X' for groups of 32"""
    n = len(X)
    if order == 0:
        Xp = list(X)
    else:
        d = [X[k] - X[k - 1] for k in range(1, n)] if order == 1 else [X[k] - 2 * X[k - 1] + X[k - 2] for k in range(2, n)]
        gmin = min(d) if d else 0
        Xp = [0] * min(order, n) + [v - gmin for v in d]
    return max(min(Xp[b:b + GROUP]) for b in range(0, n, GROUP)).bit_length()


def payload_of(X, order):
    """(the numbers of the independent encoder, its payload, its X') for the integers X in groups of 32"""
    return cases.encode(X, order, range(0, len(X), GROUP), nbytes=4, ref_bits=reference_bits(X, order), w_bits=6, l_ref=32, l_inc=1, l_bits=0)


def capacity(N, nbits, order):
    ng = (N + GROUP - 1) // GROUP
    return ((4 * (order + 1) if order else 0) + 4 * ng + (6 * ng + 7) // 8 + 4 * ng * (nbits + order) + 3) // 4 * 4


def expected_field(v, D, nbits, order):
    """v fp32 in stream order -> (vmin, vmax, R, E, bad, X or None, numbers or None, payload: b"" for a field with bad > 0)"""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    if v.size == 1:   # the restated packer takes two values or more: the same value twice has the same range, R, E and integer
        vmin, vmax, R, E, bad, stream = ref.pack(np.repeat(v, 2), D, nbits)
        bad //= 2
    else:
        vmin, vmax, R, E, bad, stream = ref.pack(v, D, nbits)
    if stream is None:
        return vmin, vmax, R, E, bad, None, None, b""
    X = integers(stream, 2 if v.size == 1 else v.size, nbits)[:v.size]
    numbers, payload, _ = payload_of(X, order)
    return vmin, vmax, R, E, bad, X, numbers, payload


def expected_call(pred, std, mean, spec, samples, features, h, w, flip):
    """pred (B,T,N,F) float32 numpy -> params (n,T,K,11) int32, payloads[(i,t,k)] and the integers X[(i,t,k)] (None with bad > 0).
    Words 5 .. 8 of a field with bad > 0 are left 0 here and are not compared."""
    pred, std, mean = (np.asarray(a, dtype=np.float32) for a in (pred, std, mean))
    n, T, K = len(samples), pred.shape[1], len(features)
    params, payloads, ints, at = np.zeros((n, T, K, PARAMS), dtype=np.int32), {}, {}, 0
    for i, b in enumerate(samples):
        for t in range(T):
            for k, f in enumerate(features):
                a = (pred[b, t, :, f] * std[f]).astype(np.float32)
                v = (a + mean[f]).astype(np.float32).reshape(h, w)
                v = v[::-1] if flip else v
                vmin, vmax, R, E, bad, X, numbers, payload = expected_field(v, *spec[k])
                params[i, t, k, :3] = np.array([vmin, vmax, R], dtype=np.float32).view(np.int32)
                params[i, t, k, 3:5] = (E, bad)
                if numbers is not None:
                    params[i, t, k, 5:9] = (numbers["ival1"], numbers["ival2"], numbers["gmin"], numbers["ref_bits"])
                params[i, t, k, 9:] = (len(payload), at)
                payloads[i, t, k], ints[i, t, k] = payload, X
                at += (len(payload) + 3) // 4 * 4
    return params, payloads, ints


def message_of(ni, nj, X, order, R, E, D, present=None):
    """a whole 5.2 / 5.3 message around the integers X, by the independent encoder"""
    numbers, payload, _ = payload_of(X, order)
    return cases.assemble(ni, nj, cases.section5(len(X), R, E, D, numbers), payload, present)


def growing_noise(n, nbits, seed=3):
    """values whose noise amplitude grows along the stream from nothing to the whole range: a constant stretch, then wider and wider
    groups, the last ones spanning [0, 1] -- so that the group widths met run from 0 up to the widest the packing can produce"""
    g = np.random.default_rng(seed)
    x = np.arange(n, dtype=np.float64) / max(n - 1, 1)
    amplitude = np.where(x < 0.15, 0.0, ((x - 0.15) / 0.85) ** 3)
    v = 0.5 + amplitude * (g.integers(0, 2, size=n) - 0.5)
    v[-GROUP:] = np.tile([0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0], GROUP // 8)[:GROUP]   # 0 -> 1 -> 0: the extreme second difference
    return v.astype(np.float32)
