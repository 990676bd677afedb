// Forecast frames: what predict_step's save_gifs (py4cast/lightning.py:1162-1188, io/outputs.py:223-240, utils.py:112-223) draws,
// made on the device as palette indices -- one byte per pixel, the colour table never enters the kernel.
//
// The reference un-normalises the whole prediction feature by feature in place (two strided passes each), pulls one strided
// (T,H,W) block per feature to the host with a blocking copy and builds one matplotlib figure per (lead time, feature).  Here
//
//   p4c_forecast_frames   reads the normalised prediction (B,T,N,F) features-last (batch and lead-time strides as p4c_map_planes
//                         takes them) of the n accepted samples and writes, for every drawn feature k of K,
//                             frames (n,T,K,H,W) uint8   row r of a frame holds grid row H-1-r (origin="lower")
//                             vrange (n,T,K,2)   fp32    the colour range each frame was drawn with.
//
// One pixel of frame (s,t,k), feature f = features[k], display row (offset, floor, vmin, vmax):
//   v = pred * std[f], rounded; + mean[f], rounded (the two steps of p4c_unnormalize_planes: this file is built with
//       -ffp-contract=off); + offset in fp32 unless the offset is 0 (the bits stay);
//   bad  when v is not finite or v < floor (floor = -inf: none);
//   range = (vmin, vmax) as given, or -- either of them NaN -- min / max of the frame's good pixels; a frame without a good
//       pixel has the range (NaN, NaN);
//   index 255 for a bad pixel; else 0 when vmax == vmin; else x = (v - vmin) / (vmax - vmin): 0 for x < 0, 254 for x >= 1,
//       floor(255 x) between -- matplotlib's Normalize + a colormap resampled to 255 colours, entry 255 the "bad" colour.
//
// Two forms, chosen once in the host function (forecast_dense):
//   dense   the (FC_TILE points x F) block of a tile is contiguous: it is read once per pass in 16-byte loads (scalar head and tail
//           where the block does not start or end on a 16-byte boundary) and transposed through LDS.  Rows have an odd pitch, and
//           point p sits in row (p & 3) * 32 + (p >> 2), so both the range pass (a lane per feature, a row per step) and the index
//           pass (a lane per four consecutive points of one feature) read without a bank conflict inside a half wave.
//   gather  a few of many features: only the lines that hold them are touched, as map_planes_kernel does.
// Index pass: a thread makes four consecutive pixels of one feature and stores them as one 32-bit word where the four lie in one
// grid row and the destination is 4-byte aligned (always when W and H*W are multiples of 4), else as bytes.
// Range pass (only when a drawn feature auto-scales): a workgroup walks the tiles of ONE (sample, lead time) with a grid stride;
// per-wave LDS slots -> block partial in the caller's workspace -> forecast_range_final_kernel.  min / max of finite values are
// exact in any order: no atomics, two calls give the same bits.  Without an auto-scaled feature the call is one launch.
#include "common.hpp"

namespace p4c {

constexpr int FC_TILE = 128;             // grid points per loop trip of a workgroup
constexpr int FC_THREADS = 256;
constexpr int FC_MAX_BLOCKS = 1024;      // workgroups of one launch, all (sample, lead time) pairs together
constexpr int FC_MAX_FEATURES = 256;     // K: per-wave range slots in LDS
constexpr int FC_MAX_SAMPLES = 256;      // n: the accepted samples travel as a kernel argument
constexpr int FC_DENSE_MAX_F = 64;       // the dense form's LDS tile: FC_TILE x (F | 1) floats
constexpr int FC_QUADS = FC_TILE / 4;    // 32

struct FcSamples {
    int32_t b[FC_MAX_SAMPLES];
};

static inline bool forecast_dense(int K, int F) { return F <= FC_DENSE_MAX_F && 2 * K >= F; }

static inline int forecast_blocks_per_frame_set(int n, int T, int64_t N) {
    const int64_t tiles = (N + FC_TILE - 1) / FC_TILE;
    int64_t cap = FC_MAX_BLOCKS / ((int64_t)n * T);
    if (cap < 1) cap = 1;
    return (int)(tiles < cap ? tiles : cap);
}

__device__ __forceinline__ int fc_row(int p) { return ((p & 3) * FC_QUADS) | (p >> 2); }

__device__ __forceinline__ float fc_value(float x, float sd, float mu, float off) {
    const float a = x * sd;
    float v = a + mu;
    if (off != 0.0f) v = v + off;
    return v;
}

__device__ __forceinline__ bool fc_good(float v, float flo) { return fabsf(v) < INFINITY && !(v < flo); }

__device__ __forceinline__ uint32_t fc_index(float v, float flo, float vmin, float vmax) {
    if (!fc_good(v, flo) || vmin != vmin || vmax != vmax) return 255u;
    if (vmax == vmin) return 0u;
    const float num = v - vmin, den = vmax - vmin;
    const float x = num / den;
    if (!(x >= 0.0f)) return 0u;
    if (x >= 1.0f) return 254u;
    const uint32_t i = (uint32_t)(255.0f * x);
    return i > 254u ? 254u : i;
}

// src: the `len` = points * F contiguous floats of a tile -> tile_s[fc_row(p) * FP + f]
__device__ __forceinline__ void fc_load_tile(const float* __restrict__ src, int len, int F, int FP, float* tile_s, int tid) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
    int head = (4 - mis) & 3;
    if (head > len) head = len;
    const int body = (len - head) >> 2;
    if (tid < head) {
        const int p = tid / F, f = tid - p * F;
        tile_s[fc_row(p) * FP + f] = src[tid];
    }
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(src + head);
#pragma unroll 2
    for (int i = tid; i < body; i += FC_THREADS) {
        const float4 v = v4[i];
        const float e4[4] = {v.x, v.y, v.z, v.w};
        const int e = head + 4 * i;
        int p = e / F, f = e - p * F;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            tile_s[fc_row(p) * FP + f] = e4[j];
            if (++f == F) {
                f = 0;
                ++p;
            }
        }
    }
    const int done = head + 4 * body;
    if (tid < len - done) {
        const int e = done + tid, p = e / F, f = e - p * F;
        tile_s[fc_row(p) * FP + f] = src[e];
    }
}

// grid (nb, n*T): min / max of the good pixels of every auto-scaled feature over the tiles this workgroup walks
template <bool DENSE>
__global__ void __launch_bounds__(FC_THREADS)
    forecast_range_kernel(const float* __restrict__ pred, int64_t pred_bs, int64_t pred_ts, const FcSamples smp,
                          const float* __restrict__ std, const float* __restrict__ mean, const int32_t* __restrict__ feats,
                          const float* __restrict__ display, float* __restrict__ partial, int T, int64_t N, int F, int K) {
    __shared__ float tile_s[DENSE ? FC_TILE * (FC_DENSE_MAX_F + 1) : 1];
    __shared__ float lo_s[4][FC_MAX_FEATURES], hi_s[4][FC_MAX_FEATURES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int st = blockIdx.y, s = st / T, t = st - s * T;
    const float* base = pred + (int64_t)smp.b[s] * pred_bs + (int64_t)t * pred_ts;
    const int FP = F | 1;
    for (int k = lane; k < K; k += 64) {   // a wave updates only its own row: no barrier for the slots
        lo_s[wv][k] = INFINITY;
        hi_s[wv][k] = -INFINITY;
    }
    const int64_t tiles = (N + FC_TILE - 1) / FC_TILE;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t n0 = tile * FC_TILE;
        const int pts = (int)(N - n0 < FC_TILE ? N - n0 : FC_TILE);
        if constexpr (DENSE) {
            __syncthreads();   // the previous trip's readers are done
            fc_load_tile(base + n0 * F, pts * F, F, FP, tile_s, tid);
            __syncthreads();
            // wave wv takes rows wv*32 .. wv*32+31, the points 4 i + wv; a lane takes a feature: consecutive banks
            for (int k = lane; k < K; k += 64) {
                const float* d = display + 4 * k;
                if (d[2] == d[2] && d[3] == d[3]) continue;   // a given range
                const int f = feats[k];
                const float sd = std[f], mu = mean[f], off = d[0], flo = d[1];
                float lo = lo_s[wv][k], hi = hi_s[wv][k];
                for (int i = 0; i < FC_QUADS; ++i) {
                    if (4 * i + wv < pts) {
                        const float v = fc_value(tile_s[(wv * FC_QUADS + i) * FP + f], sd, mu, off);
                        if (fc_good(v, flo)) {
                            lo = fminf(lo, v);
                            hi = fmaxf(hi, v);
                        }
                    }
                }
                lo_s[wv][k] = lo;
                hi_s[wv][k] = hi;
            }
        } else {
            // thread = (point, parity of k): waves 0, 1 take the even k of points 0..63 / 64..127, waves 2, 3 the odd ones
            const int p = tid & (FC_TILE - 1);
            for (int k = tid >> 7; k < K; k += 2) {
                const float* d = display + 4 * k;
                if (d[2] == d[2] && d[3] == d[3]) continue;   // uniform over the wave
                const int f = feats[k];
                float v0 = INFINITY, v1 = -INFINITY;   // a dead lane or a bad pixel leaves both sides alone
                if (p < pts) {
                    const float v = fc_value(base[(n0 + p) * F + f], std[f], mean[f], d[0]);
                    if (fc_good(v, d[1])) v0 = v1 = v;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    v0 = fminf(v0, __shfl_xor(v0, o, 64));
                    v1 = fmaxf(v1, __shfl_xor(v1, o, 64));
                }
                if (lane == 0) {
                    lo_s[wv][k] = fminf(lo_s[wv][k], v0);
                    hi_s[wv][k] = fmaxf(hi_s[wv][k], v1);
                }
            }
        }
    }
    __syncthreads();
    float* out = partial + (((int64_t)st * gridDim.x + blockIdx.x) * K) * 2;
    for (int k = tid; k < K; k += FC_THREADS) {
        out[2 * k] = fminf(fminf(lo_s[0][k], lo_s[1][k]), fminf(lo_s[2][k], lo_s[3][k]));
        out[2 * k + 1] = fmaxf(fmaxf(hi_s[0][k], hi_s[1][k]), fmaxf(hi_s[2][k], hi_s[3][k]));
    }
}

// grid (K, n*T), one wave: the range of one auto-scaled frame over the nb block partials
__global__ void __launch_bounds__(64)
    forecast_range_final_kernel(const float* __restrict__ partial, const float* __restrict__ display, float* __restrict__ vrange,
                                int nb, int K) {
    const int lane = threadIdx.x, k = blockIdx.x, st = blockIdx.y;
    const float* d = display + 4 * k;
    if (d[2] == d[2] && d[3] == d[3]) return;   // given: the index pass writes it
    float lo = INFINITY, hi = -INFINITY;
    for (int b = lane; b < nb; b += 64) {
        const float* src = partial + (((int64_t)st * nb + b) * K + k) * 2;
        lo = fminf(lo, src[0]);
        hi = fmaxf(hi, src[1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
        const bool none = lo > hi;   // no good pixel in the frame
        vrange[((int64_t)st * K + k) * 2] = none ? NAN : lo;
        vrange[((int64_t)st * K + k) * 2 + 1] = none ? NAN : hi;
    }
}

// grid (nb, n*T).  auto_range == 0: every range is taken as given (a NaN one draws an all-bad frame), vrange is not read.
template <bool DENSE>
__global__ void __launch_bounds__(FC_THREADS)
    forecast_index_kernel(const float* __restrict__ pred, int64_t pred_bs, int64_t pred_ts, const FcSamples smp,
                          const float* __restrict__ std, const float* __restrict__ mean, const int32_t* __restrict__ feats,
                          const float* __restrict__ display, float* vrange, unsigned char* __restrict__ frames, int auto_range, int T,
                          int N, int F, int K, int H, int W) {
    __shared__ float tile_s[DENSE ? FC_TILE * (FC_DENSE_MAX_F + 1) : 1];
    const int tid = threadIdx.x;
    const int st = blockIdx.y, s = st / T, t = st - s * T;
    const float* base = pred + (int64_t)smp.b[s] * pred_bs + (int64_t)t * pred_ts;
    const int FP = F | 1;
    float* vr = vrange + (int64_t)st * K * 2;
    if (blockIdx.x == 0) {   // the given ranges, as drawn; nobody reads these elements
        for (int k = tid; k < K; k += FC_THREADS) {
            const float lo = display[4 * k + 2], hi = display[4 * k + 3];
            if (!auto_range || (lo == lo && hi == hi)) {
                vr[2 * k] = lo;
                vr[2 * k + 1] = hi;
            }
        }
    }
    const int tiles = (N + FC_TILE - 1) / FC_TILE;
    const int units = K * FC_QUADS;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int n0 = tile * FC_TILE;
        const int pts = N - n0 < FC_TILE ? N - n0 : FC_TILE;
        if constexpr (DENSE) {
            __syncthreads();
            fc_load_tile(base + (int64_t)n0 * F, pts * F, F, FP, tile_s, tid);
            __syncthreads();
        }
        for (int u = tid; u < units; u += FC_THREADS) {
            const int k = u / FC_QUADS, q = u - k * FC_QUADS, p0 = 4 * q;
            if (p0 >= pts) continue;
            const float* d = display + 4 * k;
            const int f = feats[k];
            const float sd = std[f], mu = mean[f], off = d[0], flo = d[1];
            float vmin = d[2], vmax = d[3];
            if (auto_range && (vmin != vmin || vmax != vmax)) {
                vmin = vr[2 * k];
                vmax = vr[2 * k + 1];
            }
            uint32_t b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                b[j] = 255u;
                if (p0 + j < pts) {
                    float x;
                    if constexpr (DENSE) {
                        x = tile_s[(j * FC_QUADS + q) * FP + f];
                    } else {
                        x = base[(int64_t)(n0 + p0 + j) * F + f];
                    }
                    b[j] = fc_index(fc_value(x, sd, mu, off), flo, vmin, vmax);
                }
            }
            const int g = n0 + p0, y = g / W, x0 = g - y * W;
            unsigned char* frame = frames + ((size_t)st * K + k) * (size_t)N;
            unsigned char* dst = frame + (size_t)(H - 1 - y) * W + x0;
            if (p0 + 4 <= pts && x0 + 4 <= W && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
                *reinterpret_cast<uint32_t*>(dst) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (p0 + j < pts) {
                        const int gj = g + j, yj = gj / W, xj = gj - yj * W;
                        frame[(size_t)(H - 1 - yj) * W + xj] = (unsigned char)b[j];
                    }
                }
            }
        }
    }
}

}  // namespace p4c

using namespace p4c;

extern "C" int p4c_forecast_tile(void) { return FC_TILE; }
extern "C" int p4c_forecast_max_blocks(void) { return FC_MAX_BLOCKS; }
extern "C" int p4c_forecast_max_features(void) { return FC_MAX_FEATURES; }
extern "C" int p4c_forecast_max_samples(void) { return FC_MAX_SAMPLES; }
extern "C" int p4c_forecast_frames_dense(int K, int F) { return forecast_dense(K, F) ? 1 : 0; }

extern "C" size_t p4c_forecast_frames_workspace_bytes(int n, int T, int64_t N, int K) {
    if (n < 1 || T < 1 || N < 1 || K < 1) return 0;
    return (size_t)n * (size_t)T * (size_t)forecast_blocks_per_frame_set(n, T, N) * (size_t)K * 2 * sizeof(float);
}

extern "C" int p4c_forecast_frames(const float* pred, int64_t pred_bs, int64_t pred_ts, const int32_t* samples, const float* std,
                                   const float* mean, const int32_t* features, const float* display, int auto_range,
                                   unsigned char* frames, float* vrange, void* workspace, int B, int n, int T, int H, int W, int F,
                                   int K, p4c_stream_t stream) {
    P4C_CHECK_ARG(pred && samples && std && mean && features && display && frames && vrange, "p4c_forecast_frames: null pointer");
    P4C_CHECK_ARG(!auto_range || workspace, "p4c_forecast_frames: null workspace with an auto-scaled feature");
    P4C_CHECK_ARG(B > 0 && n > 0 && n <= FC_MAX_SAMPLES && T > 0 && H > 0 && W > 0 && F > 0 && (int64_t)n * T <= 65535,
                  "p4c_forecast_frames: bad dims (B=%d n=%d T=%d H=%d W=%d F=%d; n <= %d, n*T <= 65535)", B, n, T, H, W, F,
                  FC_MAX_SAMPLES);
    P4C_CHECK_ARG(K > 0 && K <= FC_MAX_FEATURES, "p4c_forecast_frames: %d features: 1 .. at most %d per call", K, FC_MAX_FEATURES);
    P4C_CHECK_ARG((reinterpret_cast<uintptr_t>(frames) & 3) == 0, "p4c_forecast_frames: frames must be 4-byte aligned");
    const int64_t N = (int64_t)H * W;
    // n*T <= 65535, K <= 256, N < 2^31: the product stays far below 2^63
    P4C_CHECK_ARG(N < ((int64_t)1 << 31) && (int64_t)n * T * K * N < ((int64_t)1 << 31),
                  "p4c_forecast_frames: %lld pixels: at most 2^31 - 1 per call", (long long)((int64_t)n * T * K * N));
    FcSamples smp;
    for (int i = 0; i < n; ++i) {
        P4C_CHECK_ARG(samples[i] >= 0 && samples[i] < B, "p4c_forecast_frames: sample %d of a batch of %d", (int)samples[i], B);
        smp.b[i] = samples[i];
    }
    for (int i = n; i < FC_MAX_SAMPLES; ++i) smp.b[i] = 0;
    // THE rule of the two forms: the dense one reads all F features of a point (4 F bytes), the gather one a memory line per drawn
    // feature and point unless neighbours share it; with at least half of the features drawn -- and a tile that fits the LDS
    // budget, F <= 64 -- the contiguous read wins, below that the undrawn columns cost more than the scattered lines
    const bool dense = forecast_dense(K, F);
    const int nb = forecast_blocks_per_frame_set(n, T, N);
    const dim3 grid((unsigned)nb, (unsigned)(n * T)), block(FC_THREADS);
    hipStream_t st = as_stream(stream);
    if (auto_range) {
        float* partial = (float*)workspace;
        if (dense)
            hipLaunchKernelGGL(forecast_range_kernel<true>, grid, block, 0, st, pred, pred_bs, pred_ts, smp, std, mean, features, display,
                               partial, T, N, F, K);
        else
            hipLaunchKernelGGL(forecast_range_kernel<false>, grid, block, 0, st, pred, pred_bs, pred_ts, smp, std, mean, features,
                               display, partial, T, N, F, K);
        P4C_CHECK_LAUNCH("p4c_forecast_frames(range)");
        hipLaunchKernelGGL(forecast_range_final_kernel, dim3((unsigned)K, (unsigned)(n * T)), dim3(64), 0, st, (const float*)partial,
                           display, vrange, nb, K);
        P4C_CHECK_LAUNCH("p4c_forecast_frames(range finish)");
    }
    if (dense)
        hipLaunchKernelGGL(forecast_index_kernel<true>, grid, block, 0, st, pred, pred_bs, pred_ts, smp, std, mean, features, display,
                           vrange, frames, auto_range, T, (int)N, F, K, H, W);
    else
        hipLaunchKernelGGL(forecast_index_kernel<false>, grid, block, 0, st, pred, pred_bs, pred_ts, smp, std, mean, features, display,
                           vrange, frames, auto_range, T, (int)N, F, K, H, W);
    P4C_CHECK_LAUNCH("p4c_forecast_frames(index)");
    return P4C_OK;
}
