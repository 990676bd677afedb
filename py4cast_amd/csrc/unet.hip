// UNet encoder block tail (mfai's UNet: encoder_k = conv1 -> norm1 -> ReLU -> conv2 -> norm2 -> ReLU, then the 2x2 max-pool in front of the
// next level and the skip into the decoder's torch.cat((upconv_k(.), enc_k), dim=1)).
//
//   forward : one pass over the block's raw conv2 output y (B, H, W, C): a = relu(y * scale + shift) (BatchNorm from the producer's
//             statistics, p4c_bnorm_finalize), rounded to the storage type, written straight into the SKIP half of the concatenation
//             buffer (pixel stride ld, the caller points at channel C); the 2x2 / stride-2 max of the stored values -> pool (B, H/2, W/2, C).
//   backward: one pass: dA = dskip + the pooled gradient routed to its window's maximum (ties: the first maximum in the scan order
//             (0,0) (0,1) (1,0) (1,1), as torch's max_pool2d), dz = dA * relu'(a) -> dz (B, H, W, C), and the batch-norm backward sums
//             of p4c_inorm_reduce (sum dz, sum dz xhat, of dz in fp32 before its rounding to the storage type) in its partial layout
//             [blk][2][C] -> p4c_inorm_finalize_bwd, p4c_inorm_apply.
// Thread = 4 channels of one 2x2 window (16 B fp32 / 8 B bf16 per pixel); fixed-order sums (bit-identical reruns).
#include "common.hpp"

namespace p4c {
namespace unet {

template <typename T>
__global__ void __launch_bounds__(256) enc_tail_fwd_kernel(const T* __restrict__ y, const float* __restrict__ scale, const float* __restrict__ shift,
                                                           T* __restrict__ skip, int64_t ld, T* __restrict__ pool, int B, int H, int W, int C) {
    const int cq = C >> 2, Ho = H >> 1, Wo = W >> 1;
    const int64_t n = (int64_t)B * Ho * Wo * cq;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int c = (int)(g % cq) * 4;
        const int64_t win = g / cq;
        const int wo = (int)(win % Wo);
        const int64_t t = win / Wo;
        const int ho = (int)(t % Ho);
        const int64_t b = t / Ho;
        const p4c_f32x4 sc = load4f(scale + c), sh = load4f(shift + c);
        p4c_f32x4 mx;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t p = (b * H + 2 * ho + (k >> 1)) * W + 2 * wo + (k & 1);
            const p4c_f32x4 v = load4f(y + p * C + c);
            p4c_f32x4 a;
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = fmaxf(__builtin_fmaf(v[j], sc[j], sh[j]), 0.f);
            store4f(skip + p * ld + c, a);
            const p4c_f32x4 r = load4f(skip + p * ld + c);      // the stored (rounded) values: what the pool and the backward see
            if (k == 0) mx = r;
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) mx[j] = r[j] > mx[j] ? r[j] : mx[j];
            }
        }
        store4f(pool + win * C + c, mx);
    }
}

constexpr int BWD_BLOCKS_MAX = 1024;

__host__ __device__ inline int bwd_windows_per_block(int C) { return 256 / (C >> 2) > 0 ? 256 / (C >> 2) : 1; }

template <typename T>
__global__ void __launch_bounds__(256) enc_tail_bwd_kernel(const T* __restrict__ y, const T* __restrict__ act, int64_t lda, const T* __restrict__ dskip,
                                                           int64_t ldd, const T* __restrict__ dpool, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, T* __restrict__ dz, float* __restrict__ partial,
                                                           int B, int H, int W, int C) {
    extern __shared__ float red[];       // [wpb][2][C]
    const int cq = C >> 2, wpb = bwd_windows_per_block(C), Ho = H >> 1, Wo = W >> 1;
    const int lc = threadIdx.x % cq, lw = threadIdx.x / cq;
    const bool active = lw < wpb;
    const int c = lc * 4;
    const int64_t nwin = (int64_t)B * Ho * Wo;
    float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const p4c_f32x4 mu = load4f(mean + c), rs = load4f(rstd + c);
        for (int64_t win = (int64_t)blockIdx.x * wpb + lw; win < nwin; win += (int64_t)gridDim.x * wpb) {
            const int wo = (int)(win % Wo);
            const int64_t t = win / Wo;
            const int ho = (int)(t % Ho);
            const int64_t b = t / Ho;
            int64_t px[4];
            p4c_f32x4 a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                px[k] = (b * H + 2 * ho + (k >> 1)) * W + 2 * wo + (k & 1);
                a[k] = load4f(act + px[k] * lda + c);
            }
            int arg[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float m = a[0][j];
                arg[j] = 0;
#pragma unroll
                for (int k = 1; k < 4; ++k)
                    if (a[k][j] > m) { m = a[k][j]; arg[j] = k; }
            }
            const p4c_f32x4 gp = load4f(dpool + win * C + c);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const p4c_f32x4 gs = load4f(dskip + px[k] * ldd + c), v = load4f(y + px[k] * C + c);
                p4c_f32x4 d;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float da = gs[j] + (arg[j] == k ? gp[j] : 0.f);
                    d[j] = a[k][j] > 0.f ? da : 0.f;
                }
                store4f(dz + px[k] * C + c, d);
                // the sums take dz before it is rounded to the storage type: dgamma / dbeta are the sums of the exact dskip + routed dpool
                // (summing the stored bf16 values instead put ~2^-9 relative noise per routed element into them, 3e-3 in the 2-norm)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s0[j] += d[j];
                    s1[j] = __builtin_fmaf(d[j], (v[j] - mu[j]) * rs[j], s1[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            red[(lw * 2 + 0) * C + c + j] = s0[j];
            red[(lw * 2 + 1) * C + c + j] = s1[j];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * C; e += 256) {
        const int which = e / C, cc = e - which * C;
        float tsum = 0.f;
        for (int r = 0; r < wpb; ++r) tsum += red[(r * 2 + which) * C + cc];
        partial[((int64_t)blockIdx.x * 2 + which) * C + cc] = tsum;
    }
}

}  // namespace unet
}  // namespace p4c

using namespace p4c;

extern "C" int p4c_unet_enc_tail_fwd(const void* y, const float* scale, const float* shift, void* skip, int64_t ld, void* pool, int dtype, int B,
                                     int H, int W, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(y && scale && shift && skip && pool, "p4c_unet_enc_tail_fwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 4 == 0 && C <= 1024 && ld >= C && ld % 4 == 0,
                  "p4c_unet_enc_tail_fwd: B=%d H=%d W=%d C=%d ld=%lld (even grid, C a multiple of 4 up to 1024)", B, H, W, C, (long long)ld);
    const int64_t n = (int64_t)B * (H / 2) * (W / 2) * (C / 4);
    const int blocks = (int)((n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536);
    hipStream_t st = as_stream(stream);
    if (dtype == P4C_F32)
        hipLaunchKernelGGL(unet::enc_tail_fwd_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)y, scale, shift, (float*)skip, ld,
                           (float*)pool, B, H, W, C);
    else if (dtype == P4C_BF16)
        hipLaunchKernelGGL(unet::enc_tail_fwd_kernel<bf16>, dim3(blocks), dim3(256), 0, st, (const bf16*)y, scale, shift, (bf16*)skip, ld,
                           (bf16*)pool, B, H, W, C);
    else return fail(P4C_ERR_INVALID, "p4c_unet_enc_tail_fwd: bad dtype");
    P4C_CHECK_LAUNCH("p4c_unet_enc_tail_fwd");
    return P4C_OK;
}

extern "C" int p4c_unet_enc_tail_bwd_blocks(int B, int H, int W, int C) {
    if (B <= 0 || H < 2 || W < 2 || C < 4) return 0;
    const int64_t nwin = (int64_t)B * (H / 2) * (W / 2);
    const int wpb = unet::bwd_windows_per_block(C);
    const int64_t need = (nwin + wpb - 1) / wpb;
    return (int)(need < unet::BWD_BLOCKS_MAX ? need : unet::BWD_BLOCKS_MAX);
}

extern "C" int p4c_unet_enc_tail_bwd(const void* y, const void* act, int64_t lda, const void* dskip, int64_t ldd, const void* dpool, const float* mean,
                                     const float* rstd, void* dz, float* partial, int dtype, int B, int H, int W, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(y && act && dskip && dpool && mean && rstd && dz && partial, "p4c_unet_enc_tail_bwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 4 == 0 && C <= 1024 && lda >= C && ldd >= C &&
                  lda % 4 == 0 && ldd % 4 == 0, "p4c_unet_enc_tail_bwd: B=%d H=%d W=%d C=%d", B, H, W, C);
    const int nb = p4c_unet_enc_tail_bwd_blocks(B, H, W, C);
    const size_t smem = (size_t)unet::bwd_windows_per_block(C) * 2 * C * sizeof(float);
    hipStream_t st = as_stream(stream);
    if (dtype == P4C_F32)
        hipLaunchKernelGGL(unet::enc_tail_bwd_kernel<float>, dim3(nb), dim3(256), smem, st, (const float*)y, (const float*)act, lda,
                           (const float*)dskip, ldd, (const float*)dpool, mean, rstd, (float*)dz, partial, B, H, W, C);
    else if (dtype == P4C_BF16)
        hipLaunchKernelGGL(unet::enc_tail_bwd_kernel<bf16>, dim3(nb), dim3(256), smem, st, (const bf16*)y, (const bf16*)act, lda,
                           (const bf16*)dskip, ldd, (const bf16*)dpool, mean, rstd, (bf16*)dz, partial, B, H, W, C);
    else return fail(P4C_ERR_INVALID, "p4c_unet_enc_tail_bwd: bad dtype");
    P4C_CHECK_LAUNCH("p4c_unet_enc_tail_bwd");
    return P4C_OK;
}
