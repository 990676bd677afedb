// What csrc/grib_pack.hip (template 5.0) and csrc/grib_pack_complex.hip (templates 5.2 / 5.3) share: the launch constants, the two read
// forms (dense through LDS, gather), the quantisation and the range and finish passes.  The contract is in grib_pack.hip.
#pragma once
#include <math.h>

#include "common.hpp"

namespace p4c {

constexpr int GP_TILE = 128;             // points per loop trip of a workgroup
constexpr int GP_THREADS = 256;
constexpr int GP_MAX_BLOCKS = 1024;      // workgroups of one launch, all (sample, lead time) pairs together
constexpr int GP_MAX_FEATURES = 256;     // K: per-wave range slots in LDS, the spec as a kernel argument
constexpr int GP_MAX_SAMPLES = 256;      // n: the accepted samples travel as a kernel argument
constexpr int GP_DENSE_MAX_F = 64;       // the dense form's LDS tile: GP_TILE x (F | 1) floats
constexpr int GP_OCTS = GP_TILE / 8;     // 16 groups of 8 points
constexpr int GP_PARAMS = 5;             // int32 words of a params record
constexpr int GP_MAX_D = 15;

struct GpSamples {
    int32_t b[GP_MAX_SAMPLES];
};
struct GpSpec {
    int8_t d[GP_MAX_FEATURES];
    uint8_t nbits[GP_MAX_FEATURES];
};

static __constant__ double gp_pow10[GP_MAX_D + 1] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};

static inline bool grib_dense(int K, int F) { return F <= GP_DENSE_MAX_F && 2 * K >= F; }

static inline int grib_blocks_per_field_set(int n, int T, int64_t N) {
    const int64_t tiles = (N + GP_TILE - 1) / GP_TILE;
    int64_t cap = GP_MAX_BLOCKS / ((int64_t)n * T);
    if (cap < 1) cap = 1;
    return (int)(tiles < cap ? tiles : cap);
}

__device__ __forceinline__ int gp_row(int p) { return ((p & 7) * GP_OCTS) | (p >> 3); }
__device__ __forceinline__ int gp_point(int row) { return ((row & (GP_OCTS - 1)) << 3) | (row / GP_OCTS); }

__device__ __forceinline__ float gp_value(float x, float sd, float mu) {
    const float a = x * sd;
    return a + mu;
}

__device__ __forceinline__ double gp_scaled(float v, int D) {
    return D >= 0 ? (double)v * gp_pow10[D] : (double)v / gp_pow10[-D];
}

// pw = 10^|D|, looked up once per lane: with the table read inside, the pack launch measures a quarter slower
__device__ __forceinline__ uint32_t gp_quant(float v, int D, double pw, double R, int E, double xmax) {
    const double s = D >= 0 ? (double)v * pw : (double)v / pw;
    const double d = s - R;
    const double t = ldexp(d, -E) + 0.5;
    const double x = floor(t);
    if (!(x < xmax)) return (uint32_t)xmax;   // the clamp; a NaN lands here too (its field is reported through `bad`)
    return x > 0.0 ? (uint32_t)x : 0u;
}

// src: `len` contiguous floats, whole points of F features, the first of them point p_off of the tile -> tile_s[gp_row(p) * FP + f]
__device__ __forceinline__ void gp_load_segment(const float* __restrict__ src, int len, int F, int FP, float* tile_s, int tid, int p_off) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
    int head = (4 - mis) & 3;
    if (head > len) head = len;
    const int body = (len - head) >> 2;
    if (tid < head) {
        const int p = tid / F, f = tid - p * F;
        tile_s[gp_row(p_off + p) * FP + f] = src[tid];
    }
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(src + head);
#pragma unroll 2
    for (int i = tid; i < body; i += GP_THREADS) {
        const float4 v = v4[i];
        const float e4[4] = {v.x, v.y, v.z, v.w};
        const int e = head + 4 * i;
        int p = e / F, f = e - p * F;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            tile_s[gp_row(p_off + p) * FP + f] = e4[j];
            if (++f == F) {
                f = 0;
                ++p;
            }
        }
    }
    const int done = head + 4 * body;
    if (tid < len - done) {
        const int e = done + tid, p = e / F, f = e - p * F;
        tile_s[gp_row(p_off + p) * FP + f] = src[e];
    }
}

// grid (nb, n*T): min / max of the finite values and the number of the others, of every packed feature over the tiles this
// workgroup walks -> partial[(st, block, k)] = {lo, hi, bad}
template <bool DENSE>
__global__ void __launch_bounds__(GP_THREADS)
    grib_range_kernel(const float* __restrict__ pred, int64_t pred_bs, int64_t pred_ts, const GpSamples smp,
                      const float* __restrict__ std, const float* __restrict__ mean, const int32_t* __restrict__ feats,
                      float* __restrict__ partial, int T, int64_t N, int F, int K) {
    __shared__ float tile_s[DENSE ? GP_TILE * (GP_DENSE_MAX_F + 1) : 1];
    __shared__ float lo_s[4][GP_MAX_FEATURES], hi_s[4][GP_MAX_FEATURES];
    __shared__ int bad_s[4][GP_MAX_FEATURES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int st = blockIdx.y, s = st / T, t = st - s * T;
    const float* base = pred + (int64_t)smp.b[s] * pred_bs + (int64_t)t * pred_ts;
    const int FP = F | 1;
    for (int k = lane; k < K; k += 64) {   // a wave updates only its own row: no barrier for the slots
        lo_s[wv][k] = INFINITY;
        hi_s[wv][k] = -INFINITY;
        bad_s[wv][k] = 0;
    }
    const int64_t tiles = (N + GP_TILE - 1) / GP_TILE;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t n0 = tile * GP_TILE;
        const int pts = (int)(N - n0 < GP_TILE ? N - n0 : GP_TILE);
        if constexpr (DENSE) {
            __syncthreads();   // the previous trip's readers are done
            gp_load_segment(base + n0 * F, pts * F, F, FP, tile_s, tid, 0);
            __syncthreads();
            // wave wv takes rows wv*32 .. wv*32+31; a lane takes a feature: consecutive banks
            for (int k = lane; k < K; k += 64) {
                const int f = feats[k];
                const float sd = std[f], mu = mean[f];
                float lo = lo_s[wv][k], hi = hi_s[wv][k];
                int bad = bad_s[wv][k];
                for (int i = 0; i < GP_TILE / 4; ++i) {
                    const int row = wv * (GP_TILE / 4) + i;
                    if (gp_point(row) < pts) {
                        const float v = gp_value(tile_s[row * FP + f], sd, mu);
                        if (fabsf(v) < INFINITY) {
                            lo = fminf(lo, v);
                            hi = fmaxf(hi, v);
                        } else {
                            ++bad;
                        }
                    }
                }
                lo_s[wv][k] = lo;
                hi_s[wv][k] = hi;
                bad_s[wv][k] = bad;
            }
        } else {
            // thread = (point, parity of k): waves 0, 1 take the even k of points 0..63 / 64..127, waves 2, 3 the odd ones
            const int p = tid & (GP_TILE - 1);
            for (int k = tid >> 7; k < K; k += 2) {
                const int f = feats[k];
                float v0 = INFINITY, v1 = -INFINITY;   // a dead lane or a non-finite value leaves both sides alone
                int bad = 0;
                if (p < pts) {
                    const float v = gp_value(base[(n0 + p) * F + f], std[f], mean[f]);
                    if (fabsf(v) < INFINITY)
                        v0 = v1 = v;
                    else
                        bad = 1;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    v0 = fminf(v0, __shfl_xor(v0, o, 64));
                    v1 = fmaxf(v1, __shfl_xor(v1, o, 64));
                    bad += __shfl_xor(bad, o, 64);
                }
                if (lane == 0) {
                    lo_s[wv][k] = fminf(lo_s[wv][k], v0);
                    hi_s[wv][k] = fmaxf(hi_s[wv][k], v1);
                    bad_s[wv][k] += bad;
                }
            }
        }
    }
    __syncthreads();
    float* out = partial + (((int64_t)st * gridDim.x + blockIdx.x) * K) * 3;
    for (int k = tid; k < K; k += GP_THREADS) {
        out[3 * k] = fminf(fminf(lo_s[0][k], lo_s[1][k]), fminf(lo_s[2][k], lo_s[3][k]));
        out[3 * k + 1] = fmaxf(fmaxf(hi_s[0][k], hi_s[1][k]), fmaxf(hi_s[2][k], hi_s[3][k]));
        out[3 * k + 2] = __int_as_float(bad_s[0][k] + bad_s[1][k] + bad_s[2][k] + bad_s[3][k]);
    }
}

// grid (K, n*T), one wave: the nb block partials of one field -> the first five words of its params record of PARAMS words
template <int PARAMS>
__global__ void __launch_bounds__(64)
    grib_finish_kernel(const float* __restrict__ partial, const GpSpec spec, int32_t* __restrict__ params, int nb, int K) {
    const int lane = threadIdx.x, k = blockIdx.x, st = blockIdx.y;
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (int b = lane; b < nb; b += 64) {
        const float* src = partial + (((int64_t)st * nb + b) * K + k) * 3;
        lo = fminf(lo, src[0]);
        hi = fmaxf(hi, src[1]);
        bad += __float_as_int(src[2]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        bad += __shfl_xor(bad, o, 64);
    }
    if (lane == 0) {
        const bool none = lo > hi;   // no finite value in the field
        float R = 0.0f;
        int E = 0;
        if (!none) {
            const int D = spec.d[k], nbits = spec.nbits[k];
            const double smin = gp_scaled(lo, D), smax = gp_scaled(hi, D);
            R = (float)smin;
            if ((double)R > smin) R = nextafterf(R, -INFINITY);
            const double range = smax - (double)R;
            if (hi != lo && range > 0.0 && range < (double)INFINITY) {
                const double xmax = ldexp(1.0, nbits) - 1.0;
                int e;
                (void)frexp(range, &e);   // range = m 2^e, 0.5 <= m < 1: at e - nbits - 1 the scaled range is at least 2^nbits
                E = e - nbits - 1;
                while (ldexp(range, -E) > xmax) ++E;
            }
        }
        int32_t* out = params + ((int64_t)st * K + k) * PARAMS;
        out[0] = __float_as_int(none ? NAN : lo);
        out[1] = __float_as_int(none ? NAN : hi);
        out[2] = __float_as_int(R);
        out[3] = E;
        out[4] = bad;
    }
}

// the NB octets of 8 values of NB bits each (NB a multiple of 4), as NB / 4 little-endian words of the big-endian bit stream
template <int NB>
__device__ __forceinline__ void gp_store_words(unsigned char* dst, const uint32_t (&X)[8]) {
    uint32_t w[NB / 4];
#pragma unroll
    for (int j = 0; j < NB / 4; ++j) w[j] = 0u;
#pragma unroll
    for (int o = 0; o < NB; ++o) {   // octet o holds stream bits 8 o .. 8 o + 7: all of them in one value, or 4 + 4 in two
        const int first = (8 * o) / NB, left = NB - (8 * o) % NB;
        uint32_t byte;
        if (left >= 8)
            byte = (X[first] >> (left - 8)) & 0xffu;
        else
            byte = ((X[first] & 0xfu) << 4) | (X[(first + 1) & 7] >> (NB - 4));
        w[o >> 2] |= byte << (8 * (o & 3));
    }
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int j = 0; j < NB / 4; ++j) d32[j] = w[j];
}

// any width: the first `nbytes` octets of the 8 values' stream, byte by byte
__device__ __forceinline__ void gp_store_bytes(unsigned char* dst, const uint32_t (&X)[8], int nbits, int nbytes) {
    uint64_t acc = 0;
    int bits = 0, o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        acc = (acc << nbits) | X[i];
        bits += nbits;
        while (bits >= 8) {
            bits -= 8;
            if (o < nbytes) dst[o] = (unsigned char)(acc >> bits);
            ++o;
        }
    }
}

// grid (nb, n*T)
template <bool DENSE>
__global__ void __launch_bounds__(GP_THREADS)
    grib_pack_kernel(const float* __restrict__ pred, int64_t pred_bs, int64_t pred_ts, const GpSamples smp,
                     const float* __restrict__ std, const float* __restrict__ mean, const int32_t* __restrict__ feats,
                     const GpSpec spec, const int32_t* __restrict__ params, unsigned char* __restrict__ packed, int64_t pitch,
                     int flip, int T, int N, int F, int K, int H, int W) {
    __shared__ float tile_s[DENSE ? GP_TILE * (GP_DENSE_MAX_F + 1) : 1];
    const int tid = threadIdx.x;
    const int st = blockIdx.y, s = st / T, t = st - s * T;
    const float* base = pred + (int64_t)smp.b[s] * pred_bs + (int64_t)t * pred_ts;
    const int FP = F | 1;
    const int tiles = (N + GP_TILE - 1) / GP_TILE;
    const int units = K * GP_OCTS;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int q0 = tile * GP_TILE;
        const int pts = N - q0 < GP_TILE ? N - q0 : GP_TILE;
        if constexpr (DENSE) {
            __syncthreads();
            if (!flip) {
                gp_load_segment(base + (int64_t)q0 * F, pts * F, F, FP, tile_s, tid, 0);
            } else {   // one contiguous piece per grid row the tile touches
                for (int p = 0; p < pts;) {
                    const int q = q0 + p, r = q / W, x = q - r * W;
                    const int len = W - x < pts - p ? W - x : pts - p;
                    gp_load_segment(base + ((int64_t)(H - 1 - r) * W + x) * F, len * F, F, FP, tile_s, tid, p);
                    p += len;
                }
            }
            __syncthreads();
        }
        for (int u = tid; u < units; u += GP_THREADS) {
            const int k = u / GP_OCTS, j = u - k * GP_OCTS, p0 = 8 * j;
            if (p0 >= pts) continue;
            const int f = feats[k];
            const float sd = std[f], mu = mean[f];
            const int D = spec.d[k], nbits = spec.nbits[k];
            const int32_t* rec = params + ((int64_t)st * K + k) * GP_PARAMS;
            const double R = (double)__int_as_float(rec[2]);
            const int E = rec[3];
            const double pw = gp_pow10[D >= 0 ? D : -D];
            const double xmax = ldexp(1.0, nbits) - 1.0;
            const int valid = pts - p0 < 8 ? pts - p0 : 8;
            int r = 0, x = 0;
            if constexpr (!DENSE) {
                r = (q0 + p0) / W;
                x = (q0 + p0) - r * W;
            }
            uint32_t X[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                X[i] = 0u;
                if (i < valid) {
                    float raw;
                    if constexpr (DENSE) {
                        raw = tile_s[(i * GP_OCTS + j) * FP + f];
                    } else {
                        const int64_t g = flip ? (int64_t)(H - 1 - r) * W + x : (int64_t)q0 + p0 + i;
                        raw = base[g * F + f];
                        if (++x == W) {
                            x = 0;
                            ++r;
                        }
                    }
                    X[i] = gp_quant(gp_value(raw, sd, mu), D, pw, R, E, xmax);
                }
            }
            unsigned char* dst = packed + ((int64_t)st * K + k) * pitch + (int64_t)((q0 + p0) >> 3) * nbits;
            if (valid == 8) {
                switch (nbits) {
                    case 8: gp_store_words<8>(dst, X); break;
                    case 12: gp_store_words<12>(dst, X); break;
                    case 16: gp_store_words<16>(dst, X); break;
                    case 24: gp_store_words<24>(dst, X); break;
                    case 32: gp_store_words<32>(dst, X); break;
                    default: gp_store_bytes(dst, X, nbits, nbits); break;
                }
            } else {
                gp_store_bytes(dst, X, nbits, (valid * nbits + 7) >> 3);
            }
        }
    }
}
}  // namespace p4c
