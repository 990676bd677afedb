// Prediction-map frames: what PredictionTimestepPlot / PredictionEpochPlot (py4cast/plots.py:242-485) show, made on the device.
//
// The reference's MapPlot.update (plots.py:260-328) copies prediction, target and batch, multiplies the whole (B,T,H,W,F)
// prediction by the mask, rescales both whole tensors (* std + mean), takes min / max over the flattened target and then pulls
// one strided (H,W) plane per (lead time, variable, panel) to the host.  It shows n samples and K of F variables.
//
//   p4c_map_planes   reads only the K requested features of the n leading samples and writes them plane-major,
//                        planes[s,t,k,0,:] = target * std + mean          planes[s,t,k,1,:] = (pred * mask) * std + mean
//                    (separately rounded steps: this file is built with -ffp-contract=off, as unnormalize_planes_kernel), and
//                    the colour range of each (sample, variable): min / max of panel 0 over (T,N), NaN propagating like torch.min.
//   p4c_map_render   turns the planes into RGB8 frames, target left, prediction right, matplotlib's Normalize + Colormap rule
//                    and the faded border of plot_prediction (alpha = clamp(interior, 0.7, 1) over white), origin="lower".
//
// map_planes: a thread owns one grid point of a 256-point tile, so for every k its loads touch exactly the 64-byte lines that
// hold feature k of those points and its two stores are runs of 256 consecutive floats of a plane: coalesced without an LDS
// transpose (the gather is on the load side, where only the requested lines may be touched).  A workgroup walks the (t, tile)
// items of ONE sample with a grid stride; the range goes wave-reduce -> per-wave LDS slot -> block partial in the caller's
// workspace -> map_range_final_kernel.  min / max are exact in any order: no atomics, two calls give the same bits.
#include "common.hpp"

namespace p4c {

constexpr int MAP_TILE = 256;            // grid points per loop trip of a workgroup (one per thread)
constexpr int MAP_MAX_BLOCKS = 512;      // workgroups of one p4c_map_planes launch, all samples together
constexpr int MAP_MAX_FEATURES = 256;    // K: per-wave range slots in LDS
constexpr int MAP_GAP = 8;               // white columns between the two panels
constexpr int MAP_RENDER_PIXELS = 4;     // pixels per thread and trip: three 32-bit stores
constexpr int MAP_RENDER_MAX_BLOCKS = 512;

// min / max that keep a NaN once seen, whichever side it is on
__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

static inline int map_blocks_per_sample(int n, int T, int64_t N) {
    const int64_t items = (int64_t)T * ((N + MAP_TILE - 1) / MAP_TILE);
    int64_t cap = MAP_MAX_BLOCKS / n;
    if (cap < 1) cap = 1;
    return (int)(items < cap ? items : cap);
}

template <int MM>
__global__ void __launch_bounds__(MAP_TILE)
    map_planes_kernel(const float* __restrict__ pred, int64_t pred_bs, int64_t pred_ts, const float* __restrict__ target,
                      int64_t tgt_bs, int64_t tgt_ts, const void* __restrict__ mask, const float* __restrict__ std,
                      const float* __restrict__ mean, const int32_t* __restrict__ feats, float* __restrict__ planes,
                      float* __restrict__ partial, int T, int64_t N, int F, int K) {
    __shared__ float lo_s[4][MAP_MAX_FEATURES], hi_s[4][MAP_MAX_FEATURES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.y;
    for (int k = lane; k < K; k += 64) {   // a wave updates only its own row: no barrier inside the loop
        lo_s[wv][k] = INFINITY;
        hi_s[wv][k] = -INFINITY;
    }
    __syncthreads();
    const int64_t tiles = (N + MAP_TILE - 1) / MAP_TILE, items = (int64_t)T * tiles;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int t = (int)(item / tiles);
        const int64_t n = (item - (int64_t)t * tiles) * MAP_TILE + tid;
        const bool live = n < N;
        const float* p = pred + (int64_t)s * pred_bs + (int64_t)t * pred_ts + n * F;
        const float* g = target + (int64_t)s * tgt_bs + (int64_t)t * tgt_ts + n * F;
        const int64_t moff = (((int64_t)s * T + t) * N + n) * F;
        float* dst = planes + (((int64_t)s * T + t) * K) * 2 * N + n;
        for (int k = 0; k < K; ++k) {
            const int f = feats[k];
            float v0 = INFINITY, v1 = -INFINITY;   // a dead lane leaves both sides of the range alone
            if (live) {
                float tg = g[f], m = 1.0f;
                if constexpr (MM == P4C_MASK_FROM_NAN) {
                    const bool isn = tg != tg;
                    m = isn ? 0.0f : 1.0f;
                    if (isn) tg = 0.0f;
                } else if constexpr (MM == P4C_MASK_F32) {
                    m = ((const float*)mask)[moff + f];
                } else if constexpr (MM == P4C_MASK_U8) {
                    m = ((const unsigned char*)mask)[moff + f] ? 1.0f : 0.0f;
                }
                const float sd = std[f], mu = mean[f];
                const float a = tg * sd;
                const float pm = p[f] * m;            // plots.py:271
                const float b = pm * sd;              // plots.py:299-300, two rounded steps each
                v0 = v1 = a + mu;
                dst[(int64_t)(2 * k) * N] = v0;
                dst[(int64_t)(2 * k + 1) * N] = b + mu;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                v0 = nan_min(v0, __shfl_xor(v0, off, 64));
                v1 = nan_max(v1, __shfl_xor(v1, off, 64));
            }
            if (lane == 0) {
                lo_s[wv][k] = nan_min(lo_s[wv][k], v0);
                hi_s[wv][k] = nan_max(hi_s[wv][k], v1);
            }
        }
    }
    __syncthreads();
    float* out = partial + (((int64_t)s * gridDim.x + blockIdx.x) * K) * 2;
    for (int k = tid; k < K; k += MAP_TILE) {
        out[2 * k] = nan_min(nan_min(lo_s[0][k], lo_s[1][k]), nan_min(lo_s[2][k], lo_s[3][k]));
        out[2 * k + 1] = nan_max(nan_max(hi_s[0][k], hi_s[1][k]), nan_max(hi_s[2][k], hi_s[3][k]));
    }
}

// grid: (K, n); a workgroup finishes one (sample, variable) over the nb block partials
__global__ void __launch_bounds__(256) map_range_final_kernel(const float* __restrict__ partial, float* __restrict__ vrange, int nb, int K) {
    __shared__ float lo_s[256], hi_s[256];
    const int tid = threadIdx.x, k = blockIdx.x, s = blockIdx.y;
    float lo = INFINITY, hi = -INFINITY;
    for (int b = tid; b < nb; b += 256) {
        const float* src = partial + (((int64_t)s * nb + b) * K + k) * 2;
        lo = nan_min(lo, src[0]);
        hi = nan_max(hi, src[1]);
    }
    lo_s[tid] = lo;
    hi_s[tid] = hi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            lo_s[tid] = nan_min(lo_s[tid], lo_s[tid + w]);
            hi_s[tid] = nan_max(hi_s[tid], hi_s[tid + w]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        vrange[((int64_t)s * K + k) * 2] = lo_s[0];
        vrange[((int64_t)s * K + k) * 2 + 1] = hi_s[0];
    }
}

// One pixel of a frame as 0x00BBGGRR.  px: the flat pixel index over (frame, row, column), frame = (s*T + t)*K + k.
__device__ __forceinline__ uint32_t map_pixel(uint32_t px, const float* __restrict__ planes, const float* __restrict__ vrange,
                                              const unsigned char* lut_s, const float* __restrict__ interior, uint32_t H, uint32_t W,
                                              uint32_t TK, uint32_t K) {
    const uint32_t RW = 2 * W + MAP_GAP;
    const uint32_t frame = px / (H * RW), rem = px - frame * (H * RW);
    const uint32_t r = rem / RW, c = rem - r * RW;
    if (c >= W && c < W + MAP_GAP) return 0x00ffffffu;
    const uint32_t panel = c < W ? 0u : 1u;
    const uint32_t idx = (H - 1 - r) * W + (panel ? c - W - MAP_GAP : c);   // origin="lower"
    const int64_t N = (int64_t)H * W;
    const float v = planes[((int64_t)frame * 2 + panel) * N + idx];
    const uint32_t s = frame / TK, k = frame % K;
    const float vmin = vrange[(s * K + k) * 2], vmax = vrange[(s * K + k) * 2 + 1];
    if (v != v || vmin != vmin || vmax != vmax) return 0x00ffffffu;
    float x = 0.0f;
    if (vmax != vmin) {
        const float num = v - vmin, den = vmax - vmin;
        x = num / den;
        if (x != x) return 0x00ffffffu;   // an infinite range
    }
    const int ci = x < 0.0f ? 0 : (x >= 1.0f ? 255 : (int)(256.0f * x));
    const float a = fminf(fmaxf(interior[idx], 0.7f), 1.0f);   // plots.py:134
    const float back = (1.0f - a) * 255.0f;
    uint32_t rgb = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float fore = a * (float)lut_s[3 * ci + ch];
        const float sum = fore + back;
        rgb |= (uint32_t)floorf(sum + 0.5f) << (8 * ch);
    }
    return rgb;
}

// A thread makes MAP_RENDER_PIXELS = 4 consecutive pixels of the flat (frames, H, 2W+G, 3) byte array -- 12 bytes, three aligned
// 32-bit stores; four pixels may straddle rows and frames, every pixel finds its own.  The last total % 4 pixels leave as bytes.
__global__ void __launch_bounds__(256)
    map_render_kernel(const float* __restrict__ planes, const float* __restrict__ vrange, const unsigned char* __restrict__ lut,
                      const float* __restrict__ interior, unsigned char* __restrict__ out, uint32_t total, uint32_t H, uint32_t W,
                      uint32_t TK, uint32_t K) {
    __shared__ unsigned char lut_s[768];
    for (int i = threadIdx.x; i < 768; i += 256) lut_s[i] = lut[i];
    __syncthreads();
    const uint32_t quads = (total + MAP_RENDER_PIXELS - 1) / MAP_RENDER_PIXELS;
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < quads; q += gridDim.x * 256u) {
        const uint32_t p0 = q * MAP_RENDER_PIXELS;
        if (p0 + MAP_RENDER_PIXELS <= total) {
            uint32_t c[MAP_RENDER_PIXELS];
#pragma unroll
            for (int j = 0; j < MAP_RENDER_PIXELS; ++j) c[j] = map_pixel(p0 + j, planes, vrange, lut_s, interior, H, W, TK, K);
            uint32_t* o = reinterpret_cast<uint32_t*>(out) + (size_t)q * 3;
            o[0] = c[0] | (c[1] << 24);
            o[1] = (c[1] >> 8) | (c[2] << 16);
            o[2] = (c[2] >> 16) | (c[3] << 8);
        } else {
            for (uint32_t px = p0; px < total; ++px) {
                const uint32_t c = map_pixel(px, planes, vrange, lut_s, interior, H, W, TK, K);
                out[(size_t)px * 3] = (unsigned char)(c & 0xff);
                out[(size_t)px * 3 + 1] = (unsigned char)((c >> 8) & 0xff);
                out[(size_t)px * 3 + 2] = (unsigned char)((c >> 16) & 0xff);
            }
        }
    }
}

}  // namespace p4c

using namespace p4c;

extern "C" int p4c_map_tile(void) { return MAP_TILE; }
extern "C" int p4c_map_max_blocks(void) { return MAP_MAX_BLOCKS; }
extern "C" int p4c_map_gap(void) { return MAP_GAP; }

extern "C" size_t p4c_map_planes_workspace_bytes(int n, int T, int64_t N, int K) {
    if (n < 1 || T < 1 || N < 1 || K < 1) return 0;
    return (size_t)n * (size_t)map_blocks_per_sample(n, T, N) * (size_t)K * 2 * sizeof(float);
}

extern "C" int p4c_map_planes(const float* pred, int64_t pred_bs, int64_t pred_ts, const float* target, int64_t tgt_bs,
                              int64_t tgt_ts, const void* mask, int mask_mode, const float* std, const float* mean,
                              const int32_t* features, float* planes, float* vrange, void* workspace, int n, int T, int64_t N, int F,
                              int K, p4c_stream_t stream) {
    P4C_CHECK_ARG(pred && target && std && mean && features && planes && vrange && workspace, "p4c_map_planes: null pointer");
    P4C_CHECK_ARG(n > 0 && n <= 65535 && T > 0 && N > 0 && N < ((int64_t)1 << 31) && F > 0,
                  "p4c_map_planes: bad dims (n=%d T=%d N=%lld F=%d)", n, T, (long long)N, F);
    P4C_CHECK_ARG(K > 0 && K <= MAP_MAX_FEATURES, "p4c_map_planes: %d features: 1 .. at most %d per call", K, MAP_MAX_FEATURES);
    P4C_CHECK_ARG(mask_mode >= P4C_MASK_NONE && mask_mode <= P4C_MASK_U8, "p4c_map_planes: bad mask mode");
    P4C_CHECK_ARG((mask_mode != P4C_MASK_F32 && mask_mode != P4C_MASK_U8) || mask, "p4c_map_planes: null mask");
    const int nb = map_blocks_per_sample(n, T, N);
    const dim3 grid((unsigned)nb, (unsigned)n), block(MAP_TILE);
    float* partial = (float*)workspace;
#define P4C_MAP_LAUNCH(MM)                                                                                                       \
    hipLaunchKernelGGL(map_planes_kernel<MM>, grid, block, 0, as_stream(stream), pred, pred_bs, pred_ts, target, tgt_bs, tgt_ts, \
                       mask, std, mean, features, planes, partial, T, N, F, K)
    switch (mask_mode) {
        case P4C_MASK_FROM_NAN: P4C_MAP_LAUNCH(P4C_MASK_FROM_NAN); break;
        case P4C_MASK_F32: P4C_MAP_LAUNCH(P4C_MASK_F32); break;
        case P4C_MASK_U8: P4C_MAP_LAUNCH(P4C_MASK_U8); break;
        default: P4C_MAP_LAUNCH(P4C_MASK_NONE); break;
    }
#undef P4C_MAP_LAUNCH
    P4C_CHECK_LAUNCH("p4c_map_planes(planes)");
    hipLaunchKernelGGL(map_range_final_kernel, dim3((unsigned)K, (unsigned)n), dim3(256), 0, as_stream(stream),
                       (const float*)partial, vrange, nb, K);
    P4C_CHECK_LAUNCH("p4c_map_planes(range)");
    return P4C_OK;
}

extern "C" int p4c_map_render_max_blocks(void) { return MAP_RENDER_MAX_BLOCKS; }
extern "C" int p4c_map_render_pixels(void) { return MAP_RENDER_PIXELS; }

extern "C" int p4c_map_render(const float* planes, const float* vrange, const unsigned char* lut, const float* interior,
                              unsigned char* frames, int n, int T, int K, int H, int W, p4c_stream_t stream) {
    P4C_CHECK_ARG(planes && vrange && lut && interior && frames, "p4c_map_render: null pointer");
    P4C_CHECK_ARG(n > 0 && T > 0 && K > 0 && H > 0 && W > 0, "p4c_map_render: bad dims (n=%d T=%d K=%d H=%d W=%d)", n, T, K, H, W);
    P4C_CHECK_ARG((reinterpret_cast<uintptr_t>(frames) & 3) == 0, "p4c_map_render: frames must be 4-byte aligned");
    const int64_t total = (int64_t)n * T * K * H * (2 * (int64_t)W + MAP_GAP);
    P4C_CHECK_ARG(total < ((int64_t)1 << 31), "p4c_map_render: %lld pixels: at most 2^31 - 1 per call", (long long)total);
    const int64_t quads = (total + MAP_RENDER_PIXELS - 1) / MAP_RENDER_PIXELS;
    int64_t blocks = (quads + 255) / 256;
    if (blocks > MAP_RENDER_MAX_BLOCKS) blocks = MAP_RENDER_MAX_BLOCKS;
    hipLaunchKernelGGL(map_render_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), planes, vrange, lut, interior,
                       frames, (uint32_t)total, (uint32_t)H, (uint32_t)W, (uint32_t)(T * K), (uint32_t)K);
    P4C_CHECK_LAUNCH("p4c_map_render");
    return P4C_OK;
}
