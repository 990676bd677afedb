// The ResNet stem tail -- BatchNorm + ReLU + the 3x3 / stride-2 / padding-1 max-pool of the stem convolution's raw output in one pass each
// way -- shared by csrc/deeplab.hip (SKIP = false: the pre-pool map is never written) and csrc/customunet.hip (SKIP = true: the activated
// map is one more output, its gradient one more input).  Features-last bf16 storage, fp32 arithmetic, sums in a fixed order.
//
//   forward  : a = relu(y * scale + shift) (BatchNorm from the producer's statistics, p4c_bnorm_finalize), rounded to bf16, and the max-pool
//              of it (padding value -inf); the window's first maximum in row-major order (torch's choice) is kept as a byte per output
//              element.  SKIP: the thread of pooled output (oy, ox) also stores a at the four pixels (2 oy + {0, 1}, 2 ox + {0, 1}) of its
//              window -- every pixel belongs to exactly one window that way -- into rows of stride ld.
//   backward : one pass per input pixel: dA = (SKIP: dskip +) the sum over the (up to 4) windows that chose this pixel of dpool, in window
//              order; dz = dA relu'(a); the batch-norm backward sums (sum dz, sum dz xhat) in the partial layout [blk][2][C] of
//              p4c_inorm_reduce -> p4c_inorm_finalize_bwd, p4c_inorm_apply.
#pragma once
#include "common.hpp"

namespace p4c {
namespace stem {

__device__ __forceinline__ float rbf(float v) { return __bfloat162float(__float2bfloat16(v)); }

// thread = 4 channels of one pooled output
template <bool SKIP>
__global__ void __launch_bounds__(256) tail_fwd_kernel(const bf16* __restrict__ y, const float* __restrict__ scale, const float* __restrict__ shift,
                                                       bf16* __restrict__ skip, int64_t ld, bf16* __restrict__ pool, unsigned char* __restrict__ arg,
                                                       int B, int H, int W, int C, int Ho, int Wo) {
    const int cq = C >> 2;
    const int64_t n = (int64_t)B * Ho * Wo * cq;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int c = (int)(g % cq) * 4;
        const int64_t win = g / cq;
        const int ox = (int)(win % Wo);
        const int64_t t = win / Wo;
        const int oy = (int)(t % Ho);
        const int64_t b = t / Ho;
        const p4c_f32x4 sc = load4f(scale + c), sh = load4f(shift + c);
        float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int am[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int iy = 2 * oy - 1 + k / 3, ix = 2 * ox - 1 + k % 3;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            const int64_t p = (b * H + iy) * W + ix;
            const p4c_f32x4 v = load4f(y + p * C + c);
            p4c_f32x4 a;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] = rbf(fmaxf(__builtin_fmaf(v[j], sc[j], sh[j]), 0.f));     // the stored value the library route would pool
                if (a[j] > mx[j]) { mx[j] = a[j]; am[j] = k; }
            }
            if constexpr (SKIP)
                if (k / 3 >= 1 && k % 3 >= 1) store4f(skip + p * ld + c, a);
        }
        store4f(pool + win * C + c, p4c_f32x4{mx[0], mx[1], mx[2], mx[3]});
        const unsigned int packed = (unsigned)am[0] | ((unsigned)am[1] << 8) | ((unsigned)am[2] << 16) | ((unsigned)am[3] << 24);
        *reinterpret_cast<unsigned int*>(arg + win * C + c) = packed;
    }
}

constexpr int BWD_BLOCKS_MAX = 1024;
__host__ __device__ inline int bwd_pixels_per_block(int C) { return 256 / (C >> 2) > 0 ? 256 / (C >> 2) : 1; }

inline int bwd_blocks(int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C < 4) return 0;
    const int64_t npix = (int64_t)B * H * W;
    const int ppb = bwd_pixels_per_block(C);
    const int64_t need = (npix + ppb - 1) / ppb;
    return (int)(need < BWD_BLOCKS_MAX ? need : BWD_BLOCKS_MAX);
}

template <bool SKIP>
__global__ void __launch_bounds__(256) tail_bwd_kernel(const bf16* __restrict__ y, const bf16* __restrict__ dskip, int64_t ld,
                                                       const bf16* __restrict__ dpool, const unsigned char* __restrict__ arg,
                                                       const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, bf16* __restrict__ dz, float* __restrict__ partial, int B, int H,
                                                       int W, int C, int Ho, int Wo) {
    extern __shared__ float red[];       // [ppb][2][C]
    const int cq = C >> 2, ppb = bwd_pixels_per_block(C);
    const int lc = threadIdx.x % cq, lp = threadIdx.x / cq;
    const bool active = lp < ppb;
    const int c = lc * 4;
    const int64_t npix = (int64_t)B * H * W;
    float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const p4c_f32x4 sc = load4f(scale + c), sh = load4f(shift + c), mu = load4f(mean + c), rs = load4f(rstd + c);
        for (int64_t p = (int64_t)blockIdx.x * ppb + lp; p < npix; p += (int64_t)gridDim.x * ppb) {
            const int ix = (int)(p % W);
            const int64_t t = p / W;
            const int iy = (int)(t % H);
            const int64_t b = t / H;
            float da[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (SKIP) {
                const p4c_f32x4 gs = load4f(dskip + p * ld + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) da[j] = gs[j];
            }
            // windows oy with 2 oy - 1 <= iy <= 2 oy + 1, in (oy, ox) order
            const int oy0 = iy / 2, oy1 = min((iy + 1) / 2, Ho - 1);
            const int ox0 = ix / 2, ox1 = min((ix + 1) / 2, Wo - 1);
            for (int oy = oy0; oy <= oy1; ++oy)
                for (int ox = ox0; ox <= ox1; ++ox) {
                    const int k = (iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1));
                    const int64_t o = ((b * Ho + oy) * Wo + ox) * C + c;
                    const unsigned int packed = *reinterpret_cast<const unsigned int*>(arg + o);
                    const p4c_f32x4 gp = load4f(dpool + o);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((int)((packed >> (8 * j)) & 0xffu) == k) da[j] += gp[j];
                }
            const p4c_f32x4 v = load4f(y + p * C + c);
            p4c_f32x4 d;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = fmaxf(__builtin_fmaf(v[j], sc[j], sh[j]), 0.f);
                d[j] = rbf(a) > 0.f ? da[j] : 0.f;
                s0[j] += d[j];
                s1[j] = __builtin_fmaf(d[j], (v[j] - mu[j]) * rs[j], s1[j]);
            }
            store4f(dz + p * C + c, d);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            red[(lp * 2 + 0) * C + c + j] = s0[j];
            red[(lp * 2 + 1) * C + c + j] = s1[j];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * C; e += 256) {
        const int which = e / C, cc = e - which * C;
        float tsum = 0.f;
        for (int r = 0; r < ppb; ++r) tsum += red[(r * 2 + which) * C + cc];
        partial[((int64_t)blockIdx.x * 2 + which) * C + cc] = tsum;
    }
}

}  // namespace stem
}  // namespace p4c
