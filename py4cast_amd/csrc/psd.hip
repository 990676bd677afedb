// Power-spectral-density validation metrics (py4cast/metrics.py:13-352: MetricPSDK, MetricPSDVar).
//
// The reference's radial_bin_dct indexes the FLATTENED variance spectrum with 2r, 2r-1 and 2r+1 (r = integer radius of a pixel),
// so a bin's value depends on r alone and reads only row 0 of the orthonormal 2-D DCT-II (indices 0 .. 2*Rmax-1) plus, for r = 0,
// index -1: the last coefficient [H-1, W-1] ("Power spectrum").  With x (B,H,W) one feature times its mask:
//   S0[b,w] = sum_h x[b,h,w]                 S1[b,w] = sum_h cH[h] x[b,h,w],   cH[h] = cos(pi (2h+1)(H-1) / (2H))
//   X[b,k]  = s_k/sqrt(H) sum_w S0[b,w] cos(pi (2w+1) k / (2W)),   s_0 = sqrt(1/W), s_k = sqrt(2/W)
//   L[b]    = sqrt(2/H) sqrt(2/W) sum_w S1[b,w] cos(pi (2w+1)(W-1) / (2W))
//   sig[k]  = mean_b X[b,k]^2 / W^2,  sigL = mean_b L[b]^2 / W^2
//   psd[q]  = sig[2q] + (q == 0 ? sigL : sig[2q-1]) / 2 + sig[2q+1] / 2                      q < Rmax
//
// psd_colsum: ONE streaming pass over prediction and target at one time step (HBM-bound, features-last rows of W*F floats); the
// rows of a slab of H are spread over the 4 waves of a block, summed in double, and one fp32 partial per (slab, b, w, f) goes to
// the workspace.  psd_finish: slab partials summed in double, the W x 2*Rmax cosine sums in double against an exact table
// (argument reduced modulo 4W in integers), mean over B, the three-term combination.  Fixed summation order, no float atomics.
#include <math.h>

#include "common.hpp"

namespace p4c {

constexpr int PSD_MAX_SLABS = 64;
constexpr int PSD_UNROLL = 4;   // rows in flight per wave and tensor

static inline bool psd_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// rows per slab (a multiple of 4: one row per wave and trip) so that about 8 blocks per CU are launched
static int psd_slab_rows(int B, int H, int64_t C, int vec) {
    const int64_t col_blocks = (C + 64 * vec - 1) / (64 * vec) * B;
    int64_t want = ((int64_t)num_cus() * 8 + col_blocks - 1) / col_blocks;
    if (want > PSD_MAX_SLABS) want = PSD_MAX_SLABS;
    if (want < 1) want = 1;
    int rs = (int)((H + want - 1) / want);
    rs = (rs + 3) / 4 * 4;
    return rs;
}

template <int VEC>
struct PsdRow {
    float p[VEC], t[VEC], m[VEC];
};

template <int VEC, int MODE>
__device__ __forceinline__ void psd_load_row(PsdRow<VEC>& r, const float* __restrict__ p, const float* __restrict__ g,
                                             const void* __restrict__ mask, int64_t e) {
    if constexpr (VEC == 4) {
        const p4c_f32x4 pv = load4f(p + e), tv = load4f(g + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) { r.p[j] = pv[j]; r.t[j] = tv[j]; r.m[j] = 1.0f; }
        if constexpr (MODE == P4C_MASK_F32) {
            const p4c_f32x4 mv = load4f((const float*)mask + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) r.m[j] = mv[j];
        }
        if constexpr (MODE == P4C_MASK_U8) {
            const unsigned int mv = *reinterpret_cast<const unsigned int*>((const unsigned char*)mask + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) r.m[j] = ((mv >> (8 * j)) & 0xffu) ? 1.0f : 0.0f;
        }
    } else {
        r.p[0] = p[e];
        r.t[0] = g[e];
        r.m[0] = 1.0f;
        if constexpr (MODE == P4C_MASK_F32) r.m[0] = ((const float*)mask)[e];
        if constexpr (MODE == P4C_MASK_U8) r.m[0] = ((const unsigned char*)mask)[e] ? 1.0f : 0.0f;
    }
}

// acc[0] pred S0, acc[1] pred S1, acc[2] target S0, acc[3] target S1
template <int VEC, int MODE>
__device__ __forceinline__ void psd_add_row(double (&acc)[4][VEC], const PsdRow<VEC>& r, float ch) {
    const double c = (double)ch;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        float tg = r.t[j], m = r.m[j];
        if constexpr (MODE == P4C_MASK_FROM_NAN) {
            m = (tg != tg) ? 0.0f : 1.0f;
            tg = (tg != tg) ? 0.0f : tg;
        }
        const double pm = (double)(r.p[j] * m), tm = (double)(tg * m);   // the reference's fp32 products (metrics.py:65-68)
        acc[0][j] += pm;
        acc[1][j] += c * pm;
        acc[2][j] += tm;
        acc[3][j] += c * tm;
    }
}

// grid (column blocks of 64*VEC, slabs, B); partial[((slab*4 + k)*B + b)*C + c]
template <int VEC, int MODE>
__global__ void __launch_bounds__(256)
    psd_colsum_kernel(const float* __restrict__ pred, int64_t pred_bs, const float* __restrict__ target, int64_t tgt_bs,
                      const void* __restrict__ mask, int64_t mask_bs, const float* __restrict__ ch, float* __restrict__ partial,
                      int H, int64_t C, int slab_rows) {
    __shared__ double red[3][4][64 * VEC];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.z, slab = blockIdx.y, B = gridDim.z;
    const int64_t c = ((int64_t)blockIdx.x * 64 + lane) * VEC;
    const bool act = c < C;   // C % VEC == 0: an active lane's VEC columns are all inside the row
    const int h0 = slab * slab_rows;
    const int h1 = (h0 + slab_rows < H) ? h0 + slab_rows : H;
    const float* p = pred + (int64_t)b * pred_bs;
    const float* g = target + (int64_t)b * tgt_bs;
    const void* mk = nullptr;
    if constexpr (MODE == P4C_MASK_F32) mk = (const float*)mask + (int64_t)b * mask_bs;
    if constexpr (MODE == P4C_MASK_U8) mk = (const unsigned char*)mask + (int64_t)b * mask_bs;
    double acc[4][VEC];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[k][j] = 0.0;
    if (act) {
        int h = h0 + wv;
        for (; h + 4 * (PSD_UNROLL - 1) < h1; h += 4 * PSD_UNROLL) {   // PSD_UNROLL rows of both tensors in flight
            PsdRow<VEC> rows[PSD_UNROLL];
#pragma unroll
            for (int u = 0; u < PSD_UNROLL; ++u) psd_load_row<VEC, MODE>(rows[u], p, g, mk, (int64_t)(h + 4 * u) * C + c);
#pragma unroll
            for (int u = 0; u < PSD_UNROLL; ++u) psd_add_row<VEC, MODE>(acc, rows[u], ch[h + 4 * u]);
        }
        for (; h < h1; h += 4) {
            PsdRow<VEC> row;
            psd_load_row<VEC, MODE>(row, p, g, mk, (int64_t)h * C + c);
            psd_add_row<VEC, MODE>(acc, row, ch[h]);
        }
    }
    if (wv > 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < VEC; ++j) red[wv - 1][k][lane * VEC + j] = acc[k][j];
    }
    __syncthreads();
    if (wv == 0 && act) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float o[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int q = lane * VEC + j;
                o[j] = (float)((acc[k][j] + red[0][k][q]) + (red[1][k][q] + red[2][k][q]));
            }
            float* dst = partial + (((int64_t)slab * 4 + k) * B + b) * C + c;
            if constexpr (VEC == 4) {
                store4f(dst, p4c_f32x4{o[0], o[1], o[2], o[3]});
            } else {
                dst[0] = o[0];
            }
        }
    }
}

__device__ __forceinline__ double psd_slab_sum(const float* __restrict__ partial, int nslab, int k, int B, int b, int64_t C,
                                               int64_t col) {
    double t = 0.0;
    for (int s = 0; s < nslab; ++s) t += (double)partial[(((int64_t)s * 4 + k) * B + b) * C + col];
    return t;
}

// cos(pi j / (2W)) for 0 <= j < 4W from the quarter-wave table tab[0..W] (tab[W] = 0)
__device__ __forceinline__ double psd_cos(const double* tab, int j, int W) {
    if (j > 2 * W) j = 4 * W - j;
    const bool neg = j > W;
    if (neg) j = 2 * W - j;
    const double v = tab[j];
    return neg ? -v : v;
}

// grid (ceil(rmax / 64), F, 2), one wave per block: lane = bin q, coefficients 2q and 2q+1; the coefficient left of the block's
// first bin (2*q0 - 1, or the corner coefficient L for q0 = 0) is summed by the whole wave.  smem: (2W + 1) doubles.
__global__ void __launch_bounds__(64)
    psd_finish_kernel(const float* __restrict__ partial, int nslab, const int32_t* __restrict__ bin_count, float* __restrict__ out,
                      int B, int H, int W, int F, int rmax) {
    extern __shared__ double psd_sm[];
    double* tab = psd_sm;
    double* s0 = psd_sm + (W + 1);
    const int lane = threadIdx.x;
    const int which = blockIdx.z, f = blockIdx.y, q0 = blockIdx.x * 64, q = q0 + lane;
    const int64_t C = (int64_t)W * F;
    const int W4 = 4 * W;
    for (int j = lane; j <= W; j += 64) tab[j] = (j == W) ? 0.0 : cospi((double)j / (2.0 * (double)W));
    const bool live = q < rmax;              // then 2q + 1 <= 2*rmax - 1 < W
    const int k0 = 2 * q, k1 = 2 * q + 1;
    const int kl = (q0 == 0) ? W - 1 : 2 * q0 - 1;
    const double sc0 = ((k0 == 0) ? sqrt(1.0 / W) : sqrt(2.0 / W)) / sqrt((double)H);
    const double sc1 = sqrt(2.0 / W) / sqrt((double)H);
    const double scl = (q0 == 0) ? sqrt(2.0 / H) * sqrt(2.0 / W) : sc1;
    double e0 = 0.0, e1 = 0.0, el = 0.0;
    for (int b = 0; b < B; ++b) {
        __syncthreads();   // the table is written; the previous sample's sums are consumed
        for (int w = lane; w < W; w += 64) s0[w] = psd_slab_sum(partial, nslab, 2 * which, B, b, C, (int64_t)w * F + f);
        __syncthreads();
        if (live) {
            double x0 = 0.0, x1 = 0.0;
            int i0 = k0, i1 = k1;                       // (2w+1) k mod 4W, advanced by 2k < 2W per step
            for (int w = 0; w < W; ++w) {
                const double v = s0[w];
                x0 += v * psd_cos(tab, i0, W);
                x1 += v * psd_cos(tab, i1, W);
                i0 += 2 * k0; if (i0 >= W4) i0 -= W4;
                i1 += 2 * k1; if (i1 >= W4) i1 -= W4;
            }
            x0 *= sc0; x1 *= sc1;
            e0 += x0 * x0; e1 += x1 * x1;
        }
        double t = 0.0;
        for (int w = lane; w < W; w += 64) {
            const double v = (q0 == 0) ? psd_slab_sum(partial, nslab, 2 * which + 1, B, b, C, (int64_t)w * F + f) : s0[w];
            t += v * psd_cos(tab, (int)(((int64_t)(2 * w + 1) * kl) % W4), W);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
        t *= scl;
        el += t * t;
    }
    const double norm = 1.0 / ((double)B * (double)W * (double)W);
    const double sig0 = e0 * norm, sig1 = e1 * norm, sigl = el * norm;
    double left = __shfl_up(sig1, 1, 64);
    if (lane == 0) left = sigl;
    if (live) {
        const double v = sig0 + 0.5 * left + 0.5 * sig1;
        out[((int64_t)which * F + f) * rmax + q] = bin_count[q] > 0 ? (float)v : __builtin_nanf("");   // 0/0 of an empty bin
    }
}

template <int VEC>
static void psd_launch_colsum(int mode, dim3 grid, hipStream_t st, const float* pred, int64_t pred_bs, const float* target,
                              int64_t tgt_bs, const void* mask, int64_t mask_bs, const float* ch, float* partial, int H, int64_t C,
                              int rs) {
    switch (mode) {
        case P4C_MASK_FROM_NAN:
            hipLaunchKernelGGL((psd_colsum_kernel<VEC, P4C_MASK_FROM_NAN>), grid, dim3(256), 0, st, pred, pred_bs, target, tgt_bs, mask,
                               mask_bs, ch, partial, H, C, rs);
            break;
        case P4C_MASK_F32:
            hipLaunchKernelGGL((psd_colsum_kernel<VEC, P4C_MASK_F32>), grid, dim3(256), 0, st, pred, pred_bs, target, tgt_bs, mask,
                               mask_bs, ch, partial, H, C, rs);
            break;
        case P4C_MASK_U8:
            hipLaunchKernelGGL((psd_colsum_kernel<VEC, P4C_MASK_U8>), grid, dim3(256), 0, st, pred, pred_bs, target, tgt_bs, mask,
                               mask_bs, ch, partial, H, C, rs);
            break;
        default:
            hipLaunchKernelGGL((psd_colsum_kernel<VEC, P4C_MASK_NONE>), grid, dim3(256), 0, st, pred, pred_bs, target, tgt_bs, mask,
                               mask_bs, ch, partial, H, C, rs);
    }
}

}  // namespace p4c

using namespace p4c;

extern "C" size_t p4c_psd_workspace_bytes(int B, int H, int W, int F) {
    if (B <= 0 || H <= 0 || W <= 0 || F <= 0) return 0;
    const int64_t C = (int64_t)W * F;
    // whichever load path p4c_psd takes (it depends on the pointers): the larger slab count of the two
    int rs = psd_slab_rows(B, H, C, 1);
    if (F % 4 == 0) { const int r4 = psd_slab_rows(B, H, C, 4); rs = r4 < rs ? r4 : rs; }
    const int nslab = (H + rs - 1) / rs;
    return (size_t)nslab * 4 * (size_t)B * (size_t)C * sizeof(float);
}

extern "C" int p4c_psd(const float* pred, int64_t pred_bs, const float* target, int64_t tgt_bs, const void* mask, int64_t mask_bs,
                       int mask_mode, const float* col_weights, const int32_t* bin_count, int rmax, float* out, void* workspace,
                       int B, int H, int W, int F, p4c_stream_t stream) {
    P4C_CHECK_ARG(pred && target && col_weights && bin_count && out && workspace, "p4c_psd: null pointer");
    P4C_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && F > 0 && F <= 256, "p4c_psd: bad dims (B=%d H=%d W=%d F=%d; F <= 256)", B, H, W, F);
    P4C_CHECK_ARG(rmax >= 1 && 2 * rmax < W, "p4c_psd: Rmax=%d: needs 1 <= Rmax and 2*Rmax < W=%d", rmax, W);
    P4C_CHECK_ARG(mask_mode >= P4C_MASK_NONE && mask_mode <= P4C_MASK_U8, "p4c_psd: bad mask mode %d", mask_mode);
    P4C_CHECK_ARG((mask_mode != P4C_MASK_F32 && mask_mode != P4C_MASK_U8) || mask, "p4c_psd: mask pointer needed");
    const size_t smem = (size_t)(2 * (int64_t)W + 1) * sizeof(double);
    P4C_CHECK_ARG(smem <= 65536, "p4c_psd: W=%d: the finish holds 2W+1 doubles in 64 KiB of LDS (W <= 4095)", W);
    const int64_t C = (int64_t)W * F;
    bool v4 = F % 4 == 0 && pred_bs % 4 == 0 && tgt_bs % 4 == 0 && psd_aligned16(pred) && psd_aligned16(target) && psd_aligned16(workspace);
    if (mask_mode == P4C_MASK_F32) v4 = v4 && mask_bs % 4 == 0 && psd_aligned16(mask);
    if (mask_mode == P4C_MASK_U8) v4 = v4 && mask_bs % 4 == 0 && (reinterpret_cast<uintptr_t>(mask) & 3u) == 0;
    const int vec = v4 ? 4 : 1;
    const int rs = psd_slab_rows(B, H, C, vec);
    const int nslab = (H + rs - 1) / rs;
    const dim3 grid((unsigned)((C + 64 * vec - 1) / (64 * vec)), nslab, B);
    hipStream_t st = as_stream(stream);
    if (v4)
        psd_launch_colsum<4>(mask_mode, grid, st, pred, pred_bs, target, tgt_bs, mask, mask_bs, col_weights, (float*)workspace, H, C, rs);
    else
        psd_launch_colsum<1>(mask_mode, grid, st, pred, pred_bs, target, tgt_bs, mask, mask_bs, col_weights, (float*)workspace, H, C, rs);
    P4C_CHECK_LAUNCH("p4c_psd(colsum)");
    hipLaunchKernelGGL(psd_finish_kernel, dim3((rmax + 63) / 64, F, 2), dim3(64), smem, st, (const float*)workspace, nslab, bin_count,
                       out, B, H, W, F, rmax);
    P4C_CHECK_LAUNCH("p4c_psd(finish)");
    return P4C_OK;
}
