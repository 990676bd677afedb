// HalfUNet with Ghost blocks (use_ghost, config/CLI/model/halfunet.yaml:22; Han et al. 2020), the bf16 route's own kernels.  All maps are
// features-last with 64 channels; storage fp32 or bf16 (a `dtype` argument), sums in fp32, every access a 16-byte vector (4 fp32 / 8 bf16
// channels per lane), no float atomics: what crosses workgroups is a per-workgroup partial the consumer sums in a fixed order, so reruns are
// bit-identical.  Nothing here allocates or synchronises.
//
//   tail_fwd      the Ghost module behind its primary convolution in ONE pass: out[..., 32 + c] = depthwise3x3(prim)[c] (zero padding),
//                 out[..., :32] = prim (skipped when prim IS out's first half), and the batch norm's sums of v and v^2 over all 64 channels
//                 of the values AS STORED, in the [blk][2][64] layout p4c_bnorm_finalize reads.
//   tail_bwd      its adjoint in ONE pass: dprim[c] = dz[c] + sum_tap w[c][tap] dz[p - tap, 32 + c] and the depthwise weight gradient's
//                 partials [blk][32][9] = sum_q prim[q, c] dz[q - tap, 32 + c] -- the SAME nine dz taps serve both, prim is read at q only.
//   merge_fwd     the decoder merge S = a0 + sum_k up_{2^k}(a_k), k = 1..4, bilinear with half-pixel centres and clamped taps
//                 (F.interpolate(scale_factor=2^k, mode="bilinear", align_corners=False)), one fp32 sum per element, rounded once.
//   merge_bwd     da_k = up_{2^k}^T dS for k = 1..4: an x pass of all four levels over dS into fp32 half-width maps tx_k, then a y pass of
//                 all four levels -- two launches, the result rounded to the storage type once.
// tail_* walk the map in tiles of th x 64 pixels (a tile row = 8 KiB of contiguous bf16 rows; th = 8, 4, 2 or 1 rows by the map's size:
// tail_tile_h), tiles dealt round-robin to the workgroups; the 3x3 halo of a tile comes from L2.
#include "common.hpp"

namespace p4c {
namespace ghost {

constexpr int CH = 32;      // channels of each half
constexpr int C = 64;
constexpr int TILE_H_MAX = 8, TILE_W = 64;

template <typename T> struct Vec;
template <> struct Vec<float> { static constexpr int N = 4; };
template <> struct Vec<bf16> { static constexpr int N = 8; };

typedef __bf16 p4c_bf16x8 __attribute__((ext_vector_type(8)));

// 16 bytes of storage <-> fp32 registers
__device__ __forceinline__ void ld16(const float* p, float (&r)[4]) {
    const p4c_f32x4 v = *reinterpret_cast<const p4c_f32x4*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = v[k];
}
__device__ __forceinline__ void ld16(const bf16* p, float (&r)[8]) {
    const p4c_bf16x8 v = *reinterpret_cast<const p4c_bf16x8*>(p);
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = (float)v[k];
}
// stores r rounded to the storage type and leaves the STORED values in r
__device__ __forceinline__ void st16(float* p, float (&r)[4]) { *reinterpret_cast<p4c_f32x4*>(p) = p4c_f32x4{r[0], r[1], r[2], r[3]}; }
__device__ __forceinline__ void st16(bf16* p, float (&r)[8]) {
    p4c_bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        o[k] = (__bf16)r[k];
        r[k] = (float)o[k];
    }
    *reinterpret_cast<p4c_bf16x8*>(p) = o;
}

// Sum over the lanes of a 16-lane row that share (lane % width), width 4 or 8, by DPP row rotations -- plain VALU adds.  (The shuffle
// form, ds_bpermute through the LDS crossbar, costs a round trip per step: 288 dependent steps made a 12 us floor under tail_bwd.)
// Afterwards every lane of the row holds its residue class's sum.
template <int CTRL>
__device__ __forceinline__ float row_rotated(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int WIDTH>
__device__ __forceinline__ float row_class_sum(float v) {
    if (WIDTH <= 4) v += row_rotated<0x124>(v);      // row_ror:4
    v += row_rotated<0x128>(v);                       // row_ror:8
    return v;
}

__host__ __device__ inline int tiles_of(int n, int t) { return (n + t - 1) / t; }

// depthwise weights (32, 9) -> LDS [tap][c]: a lane's N channels of one tap are one vector read
__device__ __forceinline__ void stage_weights(const float* __restrict__ w, float* lw) {
    for (int i = threadIdx.x; i < CH * 9; i += 256) lw[(i % 9) * CH + i / 9] = w[i];
    __syncthreads();
}

// (prim and out may be the two halves of ONE map: no __restrict__ on them)
template <typename T>
__global__ void __launch_bounds__(256) tail_fwd_kernel(const T* prim, int ldp, const float* __restrict__ w, T* out, float* __restrict__ partial,
                                                       int copy_prim, int th, int B, int H, int W) {
    constexpr int N = Vec<T>::N, NQ = CH / N, PPP = 256 / NQ;      // lanes per pixel, pixels per pass
    __shared__ __attribute__((aligned(16))) float lw[9 * CH];
    __shared__ float red[16][2 * C];          // one row per 16 lanes
    stage_weights(w, lw);
    const int q = threadIdx.x % NQ, c = q * N, pl = threadIdx.x / NQ;
    float s1p[N], s2p[N], s1c[N], s2c[N];
#pragma unroll
    for (int k = 0; k < N; ++k) s1p[k] = s2p[k] = s1c[k] = s2c[k] = 0.f;
    const int tx = tiles_of(W, TILE_W), ty = tiles_of(H, th);
    const int64_t ntiles = (int64_t)B * ty * tx;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int x0 = (int)(t % tx) * TILE_W, y0 = (int)((t / tx) % ty) * th;
        const int64_t b = t / ((int64_t)tx * ty);
        for (int i = pl; i < th * TILE_W; i += PPP) {
            const int y = y0 + i / TILE_W, x = x0 + i % TILE_W;
            if (y >= H || x >= W) continue;
            const int64_t pix = (b * H + y) * W + x;
            const T* base = prim + pix * ldp + c;
            float acc[N], ctr[N];
#pragma unroll
            for (int k = 0; k < N; ++k) acc[k] = 0.f;
#pragma unroll
            for (int ky = -1; ky <= 1; ++ky)
#pragma unroll
                for (int kx = -1; kx <= 1; ++kx) {
                    if ((unsigned)(y + ky) >= (unsigned)H || (unsigned)(x + kx) >= (unsigned)W) continue;
                    float v[N];
                    ld16(base + ((int64_t)ky * W + kx) * ldp, v);
                    const float* wt = lw + ((ky + 1) * 3 + kx + 1) * CH + c;
#pragma unroll
                    for (int k = 0; k < N; ++k) acc[k] = __builtin_fmaf(wt[k], v[k], acc[k]);
                    if (ky == 0 && kx == 0) {
#pragma unroll
                        for (int k = 0; k < N; ++k) ctr[k] = v[k];
                    }
                }
            T* o = out + pix * C;
            if (copy_prim) st16(o + c, ctr);        // (bit copy: ctr came out of the storage type)
            st16(o + CH + c, acc);                  // acc now holds what was stored
#pragma unroll
            for (int k = 0; k < N; ++k) {
                s1p[k] += ctr[k];
                s2p[k] = __builtin_fmaf(ctr[k], ctr[k], s2p[k]);
                s1c[k] += acc[k];
                s2c[k] = __builtin_fmaf(acc[k], acc[k], s2c[k]);
            }
        }
    }
    if (partial == nullptr) return;     // (uniform)
    const int row = threadIdx.x >> 4;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float a = row_class_sum<NQ>(s1p[k]), b2 = row_class_sum<NQ>(s2p[k]);
        const float d = row_class_sum<NQ>(s1c[k]), e = row_class_sum<NQ>(s2c[k]);
        if ((threadIdx.x & 15) < NQ) {
            red[row][c + k] = a;
            red[row][C + c + k] = b2;
            red[row][CH + c + k] = d;
            red[row][C + CH + c + k] = e;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * C) {
        float tsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) tsum += red[r][threadIdx.x];
        partial[(int64_t)blockIdx.x * 2 * C + threadIdx.x] = tsum;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) tail_bwd_kernel(const T* __restrict__ dz, const T* __restrict__ prim, int ldp, const float* __restrict__ w,
                                                       T* __restrict__ dprim, int ldd, float* __restrict__ wpart, int th, int B, int H, int W) {
    constexpr int N = Vec<T>::N, NQ = CH / N, PPP = 256 / NQ;
    __shared__ __attribute__((aligned(16))) float lw[9 * CH];
    __shared__ float red[16][CH * 9];         // one row per 16 lanes
    stage_weights(w, lw);
    const int q = threadIdx.x % NQ, c = q * N, pl = threadIdx.x / NQ;
    float wacc[9][N];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int k = 0; k < N; ++k) wacc[t][k] = 0.f;
    const int tx = tiles_of(W, TILE_W), ty = tiles_of(H, th);
    const int64_t ntiles = (int64_t)B * ty * tx;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int x0 = (int)(t % tx) * TILE_W, y0 = (int)((t / tx) % ty) * th;
        const int64_t b = t / ((int64_t)tx * ty);
        for (int i = pl; i < th * TILE_W; i += PPP) {
            const int y = y0 + i / TILE_W, x = x0 + i % TILE_W;
            if (y >= H || x >= W) continue;
            const int64_t pix = (b * H + y) * W + x;
            float acc[N], pv[N];
            ld16(dz + pix * C + c, acc);
            ld16(prim + pix * ldp + c, pv);
#pragma unroll
            for (int ky = -1; ky <= 1; ++ky)
#pragma unroll
                for (int kx = -1; kx <= 1; ++kx) {
                    // the output pixel p = q - tap read prim[p + tap] = prim[q]: its gradient sits at (y - ky, x - kx)
                    if ((unsigned)(y - ky) >= (unsigned)H || (unsigned)(x - kx) >= (unsigned)W) continue;
                    float g[N];
                    ld16(dz + (pix - ((int64_t)ky * W + kx)) * C + CH + c, g);
                    const int tap = (ky + 1) * 3 + kx + 1;
                    const float* wt = lw + tap * CH + c;
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        acc[k] = __builtin_fmaf(wt[k], g[k], acc[k]);
                        wacc[tap][k] = __builtin_fmaf(pv[k], g[k], wacc[tap][k]);
                    }
                }
            st16(dprim + pix * ldd + c, acc);
        }
    }
    const int row = threadIdx.x >> 4;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float s = row_class_sum<NQ>(wacc[t][k]);
            if ((threadIdx.x & 15) < NQ) red[row][(c + k) * 9 + t] = s;
        }
    __syncthreads();
    for (int e = threadIdx.x; e < CH * 9; e += 256) {
        float tsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) tsum += red[r][e];
        wpart[(int64_t)blockIdx.x * CH * 9 + e] = tsum;
    }
}

// source coordinate of fine index i at scale s = 2^k (align_corners = False): first tap, second tap (clamped), weight of the second
__device__ __forceinline__ void taps_of(int i, int s, int nk, int& i0, int& i1, float& l1) {
    const float f = fmaxf(((float)i + 0.5f) * (1.0f / (float)s) - 0.5f, 0.f);
    i0 = (int)f;
    i1 = i0 + 1 < nk ? i0 + 1 : nk - 1;
    l1 = f - (float)i0;
}

template <typename T>
struct Levels {
    T* p[4];
};

template <typename T>
__global__ void __launch_bounds__(256) merge_fwd_kernel(const T* __restrict__ a0, Levels<const T> a, T* __restrict__ out, int B, int H, int W) {
    constexpr int N = Vec<T>::N, NQ = C / N;
    const int64_t total = (int64_t)B * H * W * NQ;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % NQ) * N;
        const int64_t pix = i / NQ;
        const int x = (int)(pix % W), y = (int)((pix / W) % H);
        const int64_t b = pix / ((int64_t)W * H);
        float acc[N];
        ld16(a0 + pix * C + c, acc);
#pragma unroll
        for (int k = 1; k <= 4; ++k) {
            const int s = 1 << k, Hk = H >> k, Wk = W >> k;
            int y0, y1, x0, x1;
            float ly, lx;
            taps_of(y, s, Hk, y0, y1, ly);
            taps_of(x, s, Wk, x0, x1, lx);
            const T* base = a.p[k - 1] + b * Hk * Wk * C + c;
            float v00[N], v01[N], v10[N], v11[N];
            ld16(base + ((int64_t)y0 * Wk + x0) * C, v00);
            ld16(base + ((int64_t)y0 * Wk + x1) * C, v01);
            ld16(base + ((int64_t)y1 * Wk + x0) * C, v10);
            ld16(base + ((int64_t)y1 * Wk + x1) * C, v11);
            const float w00 = (1.f - ly) * (1.f - lx), w01 = (1.f - ly) * lx, w10 = ly * (1.f - lx), w11 = ly * lx;
#pragma unroll
            for (int j = 0; j < N; ++j)
                acc[j] += __builtin_fmaf(w11, v11[j], __builtin_fmaf(w10, v10[j], __builtin_fmaf(w01, v01[j], w00 * v00[j])));
        }
        st16(out + pix * C + c, acc);
    }
}

// fp32 intermediates of the adjoint's two passes: N floats as N / 4 16-byte accesses
template <int N>
__device__ __forceinline__ void ldf(const float* p, float (&r)[N]) {
#pragma unroll
    for (int j = 0; j < N; j += 4) {
        const p4c_f32x4 v = *reinterpret_cast<const p4c_f32x4*>(p + j);
        r[j] = v[0]; r[j + 1] = v[1]; r[j + 2] = v[2]; r[j + 3] = v[3];
    }
}
template <int N>
__device__ __forceinline__ void stf(float* p, const float (&r)[N]) {
#pragma unroll
    for (int j = 0; j < N; j += 4) *reinterpret_cast<p4c_f32x4*>(p + j) = p4c_f32x4{r[j], r[j + 1], r[j + 2], r[j + 3]};
}

// weight of fine index f on coarse index i at scale s: re-derived from the forward's own tap rule, so the clamped border taps come out as
// the forward applied them
__device__ __forceinline__ float adjoint_weight(int f, int i, int s, int nk) {
    int i0, i1;
    float l1;
    taps_of(f, s, nk, i0, i1, l1);
    return (i0 == i ? 1.f - l1 : 0.f) + (i1 == i ? l1 : 0.f);
}

// The merge's adjoint, all four levels per launch, in two passes with an fp32 intermediate (the result is rounded to the storage type once):
//   x pass  tx_k[b, y, X, :] = sum_x wx_k(x, X) dS[b, y, x, :]     tx_k (B, H, W/2^k, 64) fp32
//   y pass  da_k[b, i, X, :] = sum_y wy_k(y, i) tx_k[b, y, X, :]   da_k (B, H/2^k, W/2^k, 64)
// A lane owns one vector of one output pixel and walks the <= 2 * 2^k fine columns (rows) whose taps reach it.
template <typename T, bool XPASS>
__global__ void __launch_bounds__(256) merge_bwd_pass_kernel(const T* __restrict__ dS, Levels<float> tx, Levels<T> da, int B, int H, int W) {
    constexpr int N = Vec<T>::N, NQ = C / N;
    int64_t end[4];
    int64_t total = 0;
#pragma unroll
    for (int k = 1; k <= 4; ++k) {
        total += (int64_t)B * (XPASS ? H : H >> k) * (W >> k) * NQ;
        end[k - 1] = total;
    }
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int lvl = g < end[0] ? 0 : g < end[1] ? 1 : g < end[2] ? 2 : 3;
        // (selects, not indexed reads: a lane-varying index would put the pointer tables into scratch)
        const int64_t e = g - (lvl == 0 ? 0 : lvl == 1 ? end[0] : lvl == 2 ? end[1] : end[2]);
        float* txl = lvl == 0 ? tx.p[0] : lvl == 1 ? tx.p[1] : lvl == 2 ? tx.p[2] : tx.p[3];
        const int s = 2 << lvl, Hk = H / s, Wk = W / s;
        const int c = (int)(e % NQ) * N;
        const int64_t cp = e / NQ;
        const int X = (int)(cp % Wk);
        float acc[N];
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = 0.f;
        if (XPASS) {
            const int64_t row = cp / Wk;                     // b * H + y
            const int xlo = (X - 1) * s + s / 2 > 0 ? (X - 1) * s + s / 2 : 0;
            const int xhi = (X + 1) * s + s / 2 - 1 < W - 1 ? (X + 1) * s + s / 2 - 1 : W - 1;
            const T* src = dS + row * W * C + c;
            for (int x = xlo; x <= xhi; ++x) {
                const float wgt = adjoint_weight(x, X, s, Wk);
                float v[N];
                ld16(src + (int64_t)x * C, v);
#pragma unroll
                for (int j = 0; j < N; ++j) acc[j] = __builtin_fmaf(wgt, v[j], acc[j]);
            }
            stf<N>(txl + (row * Wk + X) * C + c, acc);
        } else {
            T* dal = lvl == 0 ? da.p[0] : lvl == 1 ? da.p[1] : lvl == 2 ? da.p[2] : da.p[3];
            const int i = (int)((cp / Wk) % Hk);
            const int64_t b = cp / ((int64_t)Wk * Hk);
            const int ylo = (i - 1) * s + s / 2 > 0 ? (i - 1) * s + s / 2 : 0;
            const int yhi = (i + 1) * s + s / 2 - 1 < H - 1 ? (i + 1) * s + s / 2 - 1 : H - 1;
            const float* src = txl + (b * H * Wk + X) * C + c;
            for (int y = ylo; y <= yhi; ++y) {
                const float wgt = adjoint_weight(y, i, s, Hk);
                float v[N];
                ldf<N>(src + (int64_t)y * Wk * C, v);
#pragma unroll
                for (int j = 0; j < N; ++j) acc[j] = __builtin_fmaf(wgt, v[j], acc[j]);
            }
            st16(dal + ((b * Hk + i) * Wk + X) * C + c, acc);
        }
    }
}

static int capped_grid(int64_t threads, int per_cu) {
    int64_t blocks = (threads + 255) / 256;
    const int64_t cap = (int64_t)num_cus() * per_cu;
    if (blocks > cap) blocks = cap;
    return (int)(blocks < 1 ? 1 : blocks);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace ghost
}  // namespace p4c

using namespace p4c;

// tile height of a launch: 8 rows where that still leaves every CU 4 workgroups, else 4, 2 or 1 -- a workgroup's passes over its tile are
// dependent memory round trips, so a small map wants many short workgroups, a large one the tall tile's halo reuse and fewer partials
static int tail_tile_h(int B, int H, int W) {
    const int64_t want = (int64_t)num_cus() * 4;
    int th = ghost::TILE_H_MAX;
    while (th > 1 && (int64_t)B * ghost::tiles_of(H, th) * ghost::tiles_of(W, ghost::TILE_W) < want) th >>= 1;
    return th;
}

extern "C" int p4c_ghost_tail_blocks(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const int64_t ntiles = (int64_t)B * ghost::tiles_of(H, tail_tile_h(B, H, W)) * ghost::tiles_of(W, ghost::TILE_W);
    const int64_t cap = (int64_t)num_cus() * 8;
    return (int)(ntiles < cap ? ntiles : cap);
}

extern "C" int p4c_ghost_tail_bwd_blocks(int B, int H, int W) { return p4c_ghost_tail_blocks(B, H, W); }

extern "C" int p4c_ghost_tail_fwd(const void* prim, int ld_prim, const float* w, void* out, int ld_out, float* partial, int dtype, int B, int H,
                                  int W, p4c_stream_t stream) {
    P4C_CHECK_ARG(prim && w && out && B > 0 && H > 0 && W > 0, "p4c_ghost_tail_fwd: bad arguments");
    P4C_CHECK_ARG((ld_prim == 32 || ld_prim == 64) && ld_out == 64, "p4c_ghost_tail_fwd: ld_prim=%d (32 or 64), ld_out=%d (64)", ld_prim, ld_out);
    P4C_CHECK_ARG(dtype == P4C_F32 || dtype == P4C_BF16, "p4c_ghost_tail_fwd: bad dtype %d", dtype);
    P4C_CHECK_ARG(ghost::aligned16(prim) && ghost::aligned16(out), "p4c_ghost_tail_fwd: maps must be 16-byte aligned");
    P4C_CHECK_ARG(prim != out || ld_prim == 64, "p4c_ghost_tail_fwd: an in-place call has ld_prim = 64");
    const int copy = prim != out;
    const int grid = p4c_ghost_tail_blocks(B, H, W);
    if (dtype == P4C_F32)
        hipLaunchKernelGGL(ghost::tail_fwd_kernel<float>, dim3(grid), dim3(256), 0, as_stream(stream), (const float*)prim, ld_prim, w, (float*)out,
                           partial, copy, tail_tile_h(B, H, W), B, H, W);
    else
        hipLaunchKernelGGL(ghost::tail_fwd_kernel<bf16>, dim3(grid), dim3(256), 0, as_stream(stream), (const bf16*)prim, ld_prim, w, (bf16*)out,
                           partial, copy, tail_tile_h(B, H, W), B, H, W);
    P4C_CHECK_LAUNCH("p4c_ghost_tail_fwd");
    return P4C_OK;
}

extern "C" int p4c_ghost_tail_bwd(const void* dz, const void* prim, int ld_prim, const float* w, void* dprim, int ld_dprim, float* wpart, int dtype,
                                  int B, int H, int W, p4c_stream_t stream) {
    P4C_CHECK_ARG(dz && prim && w && dprim && wpart && B > 0 && H > 0 && W > 0, "p4c_ghost_tail_bwd: bad arguments");
    P4C_CHECK_ARG((ld_prim == 32 || ld_prim == 64) && (ld_dprim == 32 || ld_dprim == 64), "p4c_ghost_tail_bwd: ld_prim=%d ld_dprim=%d (32 or 64)",
                  ld_prim, ld_dprim);
    P4C_CHECK_ARG(dtype == P4C_F32 || dtype == P4C_BF16, "p4c_ghost_tail_bwd: bad dtype %d", dtype);
    P4C_CHECK_ARG(ghost::aligned16(dz) && ghost::aligned16(prim) && ghost::aligned16(dprim), "p4c_ghost_tail_bwd: maps must be 16-byte aligned");
    P4C_CHECK_ARG(dprim != dz && dprim != prim, "p4c_ghost_tail_bwd: dprim must not alias its inputs");
    const int grid = p4c_ghost_tail_bwd_blocks(B, H, W);
    if (dtype == P4C_F32)
        hipLaunchKernelGGL(ghost::tail_bwd_kernel<float>, dim3(grid), dim3(256), 0, as_stream(stream), (const float*)dz, (const float*)prim, ld_prim, w,
                           (float*)dprim, ld_dprim, wpart, tail_tile_h(B, H, W), B, H, W);
    else
        hipLaunchKernelGGL(ghost::tail_bwd_kernel<bf16>, dim3(grid), dim3(256), 0, as_stream(stream), (const bf16*)dz, (const bf16*)prim, ld_prim, w,
                           (bf16*)dprim, ld_dprim, wpart, tail_tile_h(B, H, W), B, H, W);
    P4C_CHECK_LAUNCH("p4c_ghost_tail_bwd");
    return P4C_OK;
}

static int merge_shape_ok(const char* who, int dtype, int B, int H, int W, int C) {
    P4C_CHECK_ARG(dtype == P4C_F32 || dtype == P4C_BF16, "%s: bad dtype %d", who, dtype);
    P4C_CHECK_ARG(B > 0 && H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0 && C == 64,
                  "%s: B=%d H=%d W=%d C=%d (H and W multiples of 16, 64 channels)", who, B, H, W, C);
    return P4C_OK;
}

extern "C" int p4c_halfunet_merge_fwd(const void* a0, const void* a1, const void* a2, const void* a3, const void* a4, void* out, int dtype, int B,
                                      int H, int W, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(a0 && a1 && a2 && a3 && a4 && out, "p4c_halfunet_merge_fwd: NULL pointer");
    P4C_TRY(merge_shape_ok("p4c_halfunet_merge_fwd", dtype, B, H, W, C));
    P4C_CHECK_ARG(ghost::aligned16(a0) && ghost::aligned16(a1) && ghost::aligned16(a2) && ghost::aligned16(a3) && ghost::aligned16(a4) &&
                  ghost::aligned16(out), "p4c_halfunet_merge_fwd: maps must be 16-byte aligned");
    const int nq = dtype == P4C_F32 ? 16 : 8;
    const int grid = ghost::capped_grid((int64_t)B * H * W * nq, 16);
    if (dtype == P4C_F32) {
        ghost::Levels<const float> a{{(const float*)a1, (const float*)a2, (const float*)a3, (const float*)a4}};
        hipLaunchKernelGGL(ghost::merge_fwd_kernel<float>, dim3(grid), dim3(256), 0, as_stream(stream), (const float*)a0, a, (float*)out, B, H, W);
    } else {
        ghost::Levels<const bf16> a{{(const bf16*)a1, (const bf16*)a2, (const bf16*)a3, (const bf16*)a4}};
        hipLaunchKernelGGL(ghost::merge_fwd_kernel<bf16>, dim3(grid), dim3(256), 0, as_stream(stream), (const bf16*)a0, a, (bf16*)out, B, H, W);
    }
    P4C_CHECK_LAUNCH("p4c_halfunet_merge_fwd");
    return P4C_OK;
}

extern "C" int p4c_halfunet_merge_bwd(const void* dS, void* tx1, void* tx2, void* tx3, void* tx4, void* da1, void* da2, void* da3, void* da4, int dtype,
                                      int B, int H, int W, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(dS && tx1 && tx2 && tx3 && tx4 && da1 && da2 && da3 && da4, "p4c_halfunet_merge_bwd: NULL pointer");
    P4C_TRY(merge_shape_ok("p4c_halfunet_merge_bwd", dtype, B, H, W, C));
    P4C_CHECK_ARG(ghost::aligned16(dS) && ghost::aligned16(tx1) && ghost::aligned16(tx2) && ghost::aligned16(tx3) && ghost::aligned16(tx4) &&
                  ghost::aligned16(da1) && ghost::aligned16(da2) && ghost::aligned16(da3) && ghost::aligned16(da4),
                  "p4c_halfunet_merge_bwd: maps must be 16-byte aligned");
    const int nq = dtype == P4C_F32 ? 16 : 8;
    int64_t tx_threads = 0, da_threads = 0;
    for (int k = 1; k <= 4; ++k) {
        tx_threads += (int64_t)B * H * (W >> k) * nq;
        da_threads += (int64_t)B * (H >> k) * (W >> k) * nq;
    }
    const int gx = ghost::capped_grid(tx_threads, 16), gy = ghost::capped_grid(da_threads, 16);
    ghost::Levels<float> tx{{(float*)tx1, (float*)tx2, (float*)tx3, (float*)tx4}};
    hipStream_t st = as_stream(stream);
    if (dtype == P4C_F32) {
        ghost::Levels<float> da{{(float*)da1, (float*)da2, (float*)da3, (float*)da4}};
        hipLaunchKernelGGL((ghost::merge_bwd_pass_kernel<float, true>), dim3(gx), dim3(256), 0, st, (const float*)dS, tx, da, B, H, W);
        hipLaunchKernelGGL((ghost::merge_bwd_pass_kernel<float, false>), dim3(gy), dim3(256), 0, st, (const float*)dS, tx, da, B, H, W);
    } else {
        ghost::Levels<bf16> da{{(bf16*)da1, (bf16*)da2, (bf16*)da3, (bf16*)da4}};
        hipLaunchKernelGGL((ghost::merge_bwd_pass_kernel<bf16, true>), dim3(gx), dim3(256), 0, st, (const bf16*)dS, tx, da, B, H, W);
        hipLaunchKernelGGL((ghost::merge_bwd_pass_kernel<bf16, false>), dim3(gy), dim3(256), 0, st, (const bf16*)dS, tx, da, B, H, W);
    }
    P4C_CHECK_LAUNCH("p4c_halfunet_merge_bwd");
    return P4C_OK;
}
