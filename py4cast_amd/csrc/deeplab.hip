// DeepLabV3 (smp's DeepLabV3 on a dilated ResNet encoder, as mfai builds it): the passes that the GEMMs of csrc/gemm.hip do not
// cover.  Features-last bf16 storage, fp32 arithmetic, every sum in a fixed order (no atomics): reruns and graph replays are
// bit-identical.
//
//   stem tail : BatchNorm + ReLU + the 3x3 / stride-2 / padding-1 max-pool in one pass each way, the pre-pool map never written: the
//               kernels of csrc/stem_tail.hpp without their skip output.
//   col sums  : partial[b][s][c] = sum over rows s R .. s R + R - 1 of sample b of x[b][row][c] (x bf16 rows of stride ld), rows in
//               order: the ASPP pooling branch's spatial mean (forward) and the pooled column's gradient (backward).
//   pool head : the pooling branch after the mean -- z = W mean (1x1 conv, no bias, fp32), BatchNorm over the B samples (fp32: the
//               statistics of two values amplify any rounding), ReLU -> pooled (B, dc) fp32; backward: dz, dgamma, dbeta per channel,
//               then dW = dz^T mean and dmean = dz W, then the broadcast dx = dmean / (H W) over the map.
//   assemble  : the projection's input (M, 5 dc) = [a0 | a1 | a2 | a3 | broadcast pooled] -- the four spatial branches and the pooled
//               row of the pixel's sample; backward: the four column slices out into their own (M, dc) gradients.
#include "common.hpp"
#include "stem_tail.hpp"

namespace p4c {
namespace deeplab {

inline int grid_for(int64_t n) { return (int)((n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536); }

// ---------------------------------------------------------------- column sums per sample
// block = 64 columns x 4 row lanes; grid (ceil(C / 64), S, B)
__global__ void __launch_bounds__(256) colsum_kernel(const bf16* __restrict__ x, int64_t ld, float* __restrict__ partial, int HW, int C,
                                                     int rows_per_chunk) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl, s = blockIdx.y, b = blockIdx.z, S = gridDim.y;
    const int r0 = s * rows_per_chunk, r1 = min(HW, r0 + rows_per_chunk);
    float acc = 0.f;
    if (c < C) {
        const bf16* xb = x + (int64_t)b * HW * ld + c;
        for (int r = r0 + rl; r < r1; r += 4) acc += __bfloat162float(xb[(int64_t)r * ld]);
    }
    red[rl][cl] = acc;
    __syncthreads();
    if (rl == 0 && c < C) partial[((int64_t)b * S + s) * C + c] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

// ---------------------------------------------------------------- pooling branch head
// block = 64 output channels; dynamic LDS: mean (B, C) fp32
__global__ void __launch_bounds__(64) pool_head_fwd_kernel(const float* __restrict__ partial, int S, float inv_hw, const float* __restrict__ w,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float momentum,
                                                           float* __restrict__ running_mean, float* __restrict__ running_var,
                                                           long long* __restrict__ nbt, int training, int B, int C, int D,
                                                           float* __restrict__ mean_out, float* __restrict__ zsave, float* __restrict__ stat,
                                                           float* __restrict__ out) {
    extern __shared__ float mn[];        // [B][C]
    for (int e = threadIdx.x; e < B * C; e += 64) {
        const int b = e / C, c = e - b * C;
        float s = 0.f;
        for (int k = 0; k < S; ++k) s += partial[((int64_t)b * S + k) * C + c];
        mn[e] = s * inv_hw;
        if (blockIdx.x == 0) mean_out[e] = mn[e];
    }
    __syncthreads();
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= D) return;
    float z[16];
    for (int b = 0; b < B; ++b) {
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = __builtin_fmaf(w[(int64_t)o * C + c], mn[b * C + c], acc);
        z[b] = acc;
        zsave[(int64_t)b * D + o] = acc;
    }
    float mu, rstd;
    if (training) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += z[b];
        mu = s / (float)B;
        float v = 0.f;
        for (int b = 0; b < B; ++b) v = __builtin_fmaf(z[b] - mu, z[b] - mu, v);
        const float var = v / (float)B;
        rstd = 1.f / sqrtf(var + eps);
        if (running_mean) {
            running_mean[o] = (1.f - momentum) * running_mean[o] + momentum * mu;
            running_var[o] = (1.f - momentum) * running_var[o] + momentum * (v / (float)(B - 1));
        }
        if (nbt && o == 0) nbt[0] += 1;
    } else {
        mu = running_mean[o];
        rstd = 1.f / sqrtf(running_var[o] + eps);
    }
    stat[o] = mu;
    stat[D + o] = rstd;
    const float g = gamma ? gamma[o] : 1.f, bb = beta ? beta[o] : 0.f;
    for (int b = 0; b < B; ++b) out[(int64_t)b * D + o] = fmaxf(__builtin_fmaf((z[b] - mu) * rstd, g, bb), 0.f);
}

// per output channel: the gradient of the pooled row (the sum of its broadcast columns' gradients, from colsum partials), ReLU', the
// batch norm over B -> dz (B, D), dgamma, dbeta
__global__ void __launch_bounds__(64) pool_head_bwd_kernel(const float* __restrict__ gpart, int S, const float* __restrict__ zsave,
                                                           const float* __restrict__ stat, const float* __restrict__ out,
                                                           const float* __restrict__ gamma, int training, int B, int D, float* __restrict__ dz,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= D) return;
    const float mu = stat[o], rstd = stat[D + o], g = gamma ? gamma[o] : 1.f;
    float dy[16], xh[16];
    float sdy = 0.f, sdyx = 0.f;
    for (int b = 0; b < B; ++b) {
        float s = 0.f;
        for (int k = 0; k < S; ++k) s += gpart[((int64_t)b * S + k) * D + o];
        dy[b] = out[(int64_t)b * D + o] > 0.f ? s : 0.f;
        xh[b] = (zsave[(int64_t)b * D + o] - mu) * rstd;
        sdy += dy[b];
        sdyx = __builtin_fmaf(dy[b], xh[b], sdyx);
    }
    dgamma[o] = sdyx;
    dbeta[o] = sdy;
    for (int b = 0; b < B; ++b) {
        float d = dy[b] * g;
        if (training) d = d - (sdy * g) / (float)B - xh[b] * (sdyx * g) / (float)B;
        dz[(int64_t)b * D + o] = d * rstd;
    }
}

// threads [0, D C): dw[o][c] = sum_b dz[b][o] mean[b][c];  threads [D C, D C + B C): dmean[b][c] = sum_o dz[b][o] w[o][c]
__global__ void __launch_bounds__(256) pool_head_bwd2_kernel(const float* __restrict__ dz, const float* __restrict__ mean, const float* __restrict__ w,
                                                             int B, int C, int D, float* __restrict__ dw, float* __restrict__ dmean) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nw = (int64_t)D * C;
    if (i < nw) {
        const int o = (int)(i / C), c = (int)(i - (int64_t)o * C);
        float s = 0.f;
        for (int b = 0; b < B; ++b) s = __builtin_fmaf(dz[(int64_t)b * D + o], mean[(int64_t)b * C + c], s);
        dw[i] = s;
    } else if (i < nw + (int64_t)B * C) {
        const int e = (int)(i - nw), b = e / C, c = e - b * C;
        float s = 0.f;
        for (int o = 0; o < D; ++o) s = __builtin_fmaf(dz[(int64_t)b * D + o], w[(int64_t)o * C + c], s);
        dmean[e] = s;
    }
}

// dx[b][p][c] = dmean[b][c] / HW (bf16), 4 channels per thread
__global__ void __launch_bounds__(256) pool_broadcast_kernel(const float* __restrict__ dmean, float inv_hw, bf16* __restrict__ dx, int B, int HW, int C) {
    const int cq = C >> 2;
    const int64_t n = (int64_t)B * HW * cq;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int c = (int)(g % cq) * 4;
        const int64_t p = g / cq;
        const int64_t b = p / HW;
        p4c_f32x4 v = load4f(dmean + b * C + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] *= inv_hw;
        store4f(dx + p * C + c, v);
    }
}

// ---------------------------------------------------------------- ASPP projection input
// thread = 4 columns of one row of the (M, 5 D) buffer
__global__ void __launch_bounds__(256) assemble_fwd_kernel(const bf16* __restrict__ a0, const bf16* __restrict__ a1, const bf16* __restrict__ a2,
                                                           const bf16* __restrict__ a3, const float* __restrict__ pooled, bf16* __restrict__ buf,
                                                           int64_t M, int HW, int D) {
    const int cq = (5 * D) >> 2;
    const int64_t n = M * cq;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int col = (int)(g % cq) * 4;
        const int64_t m = g / cq;
        const int br = col / D, c = col - br * D;
        p4c_f32x4 v;
        if (br == 4) v = load4f(pooled + (m / HW) * D + c);
        else {
            const bf16* src = br == 0 ? a0 : br == 1 ? a1 : br == 2 ? a2 : a3;
            v = load4f(src + m * D + c);
        }
        store4f(buf + m * 5 * D + col, v);
    }
}

__global__ void __launch_bounds__(256) assemble_bwd_kernel(const bf16* __restrict__ dbuf, bf16* __restrict__ d0, bf16* __restrict__ d1,
                                                           bf16* __restrict__ d2, bf16* __restrict__ d3, int64_t M, int D) {
    const int cq = D;     // (4 D) / 4
    const int64_t n = M * cq;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int col = (int)(g % cq) * 4;
        const int64_t m = g / cq;
        const int br = col / D, c = col - br * D;
        bf16* dst = br == 0 ? d0 : br == 1 ? d1 : br == 2 ? d2 : d3;
        *reinterpret_cast<p4c_bf16x4*>(dst + m * D + c) = *reinterpret_cast<const p4c_bf16x4*>(dbuf + m * 5 * D + col);
    }
}

}  // namespace deeplab
}  // namespace p4c

using namespace p4c;

extern "C" int p4c_deeplab_stem_fwd(const void* y, const float* scale, const float* shift, void* pool, void* arg, int B, int H, int W, int C,
                                    p4c_stream_t stream) {
    P4C_CHECK_ARG(y && scale && shift && pool && arg, "p4c_deeplab_stem_fwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && C <= 1024, "p4c_deeplab_stem_fwd: B=%d H=%d W=%d C=%d (C a multiple of 4 "
                  "up to 1024)", B, H, W, C);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t n = (int64_t)B * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(stem::tail_fwd_kernel<false>, dim3(deeplab::grid_for(n)), dim3(256), 0, as_stream(stream), (const bf16*)y, scale, shift,
                       (bf16*)nullptr, (int64_t)0, (bf16*)pool, (unsigned char*)arg, B, H, W, C, Ho, Wo);
    P4C_CHECK_LAUNCH("p4c_deeplab_stem_fwd");
    return P4C_OK;
}

extern "C" int p4c_deeplab_stem_bwd_blocks(int B, int H, int W, int C) { return stem::bwd_blocks(B, H, W, C); }

extern "C" int p4c_deeplab_stem_bwd(const void* y, const void* dpool, const void* arg, const float* scale, const float* shift, const float* mean,
                                    const float* rstd, void* dz, float* partial, int B, int H, int W, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(y && dpool && arg && scale && shift && mean && rstd && dz && partial, "p4c_deeplab_stem_bwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && C <= 1024, "p4c_deeplab_stem_bwd: B=%d H=%d W=%d C=%d", B, H, W, C);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int nb = stem::bwd_blocks(B, H, W, C);
    const size_t smem = (size_t)stem::bwd_pixels_per_block(C) * 2 * C * sizeof(float);
    hipLaunchKernelGGL(stem::tail_bwd_kernel<false>, dim3(nb), dim3(256), smem, as_stream(stream), (const bf16*)y, (const bf16*)nullptr, (int64_t)0,
                       (const bf16*)dpool, (const unsigned char*)arg, scale, shift, mean, rstd, (bf16*)dz, partial, B, H, W, C, Ho, Wo);
    P4C_CHECK_LAUNCH("p4c_deeplab_stem_bwd");
    return P4C_OK;
}

extern "C" int p4c_deeplab_colsum(const void* x, int64_t ld, float* partial, int B, int HW, int C, int S, p4c_stream_t stream) {
    P4C_CHECK_ARG(x && partial, "p4c_deeplab_colsum: NULL pointer");
    P4C_CHECK_ARG(B > 0 && HW > 0 && C > 0 && ld >= C && S > 0 && S <= HW && S <= 65535 && B <= 65535, "p4c_deeplab_colsum: B=%d HW=%d C=%d S=%d",
                  B, HW, C, S);
    const int rpc = (HW + S - 1) / S;
    hipLaunchKernelGGL(deeplab::colsum_kernel, dim3((C + 63) / 64, S, B), dim3(256), 0, as_stream(stream), (const bf16*)x, ld, partial, HW, C, rpc);
    P4C_CHECK_LAUNCH("p4c_deeplab_colsum");
    return P4C_OK;
}

extern "C" int p4c_deeplab_pool_head_fwd(const float* partial, int S, int HW, const float* w, const float* gamma, const float* beta, float eps,
                                         float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, int training, int B,
                                         int C, int D, float* mean, float* z, float* stat, float* out, p4c_stream_t stream) {
    P4C_CHECK_ARG(partial && w && mean && z && stat && out, "p4c_deeplab_pool_head_fwd: NULL pointer");
    P4C_CHECK_ARG(B >= 1 && B <= 16 && (!training || B >= 2) && S > 0 && HW > 0 && C > 0 && D > 0 && (size_t)B * C * 4 <= 65536,
                  "p4c_deeplab_pool_head_fwd: B=%d (2..16 in training, 1..16 in eval) C=%d D=%d", B, C, D);
    P4C_CHECK_ARG(training || (running_mean && running_var), "p4c_deeplab_pool_head_fwd: eval needs the running statistics");
    P4C_CHECK_ARG(!running_mean == !running_var, "p4c_deeplab_pool_head_fwd: running_mean and running_var go together");
    hipLaunchKernelGGL(deeplab::pool_head_fwd_kernel, dim3((D + 63) / 64), dim3(64), (size_t)B * C * 4, as_stream(stream), partial, S, 1.f / (float)HW,
                       w, gamma, beta, eps, momentum, running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), training, B, C, D,
                       mean, z, stat, out);
    P4C_CHECK_LAUNCH("p4c_deeplab_pool_head_fwd");
    return P4C_OK;
}

extern "C" int p4c_deeplab_pool_head_bwd(const float* gpart, int S, const float* z, const float* stat, const float* out, const float* gamma,
                                         const float* mean, const float* w, int training, int B, int C, int D, float* dz, float* dgamma,
                                         float* dbeta, float* dw, float* dmean, p4c_stream_t stream) {
    P4C_CHECK_ARG(gpart && z && stat && out && mean && w && dz && dgamma && dbeta && dw && dmean, "p4c_deeplab_pool_head_bwd: NULL pointer");
    P4C_CHECK_ARG(B >= 1 && B <= 16 && S > 0 && C > 0 && D > 0, "p4c_deeplab_pool_head_bwd: B=%d C=%d D=%d", B, C, D);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(deeplab::pool_head_bwd_kernel, dim3((D + 63) / 64), dim3(64), 0, st, gpart, S, z, stat, out, gamma, training, B, D, dz, dgamma,
                       dbeta);
    P4C_CHECK_LAUNCH("p4c_deeplab_pool_head_bwd");
    const int64_t n = (int64_t)D * C + (int64_t)B * C;
    hipLaunchKernelGGL(deeplab::pool_head_bwd2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dz, mean, w, B, C, D, dw, dmean);
    P4C_CHECK_LAUNCH("p4c_deeplab_pool_head_bwd2");
    return P4C_OK;
}

extern "C" int p4c_deeplab_pool_broadcast(const float* dmean, void* dx, int B, int HW, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(dmean && dx, "p4c_deeplab_pool_broadcast: NULL pointer");
    P4C_CHECK_ARG(B > 0 && HW > 0 && C > 0 && C % 4 == 0, "p4c_deeplab_pool_broadcast: B=%d HW=%d C=%d", B, HW, C);
    const int64_t n = (int64_t)B * HW * (C / 4);
    hipLaunchKernelGGL(deeplab::pool_broadcast_kernel, dim3(deeplab::grid_for(n)), dim3(256), 0, as_stream(stream), dmean, 1.f / (float)HW, (bf16*)dx,
                       B, HW, C);
    P4C_CHECK_LAUNCH("p4c_deeplab_pool_broadcast");
    return P4C_OK;
}

extern "C" int p4c_deeplab_assemble_fwd(const void* a0, const void* a1, const void* a2, const void* a3, const float* pooled, void* buf, int B, int HW,
                                        int D, p4c_stream_t stream) {
    P4C_CHECK_ARG(a0 && a1 && a2 && a3 && pooled && buf, "p4c_deeplab_assemble_fwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && HW > 0 && D > 0 && D % 4 == 0, "p4c_deeplab_assemble_fwd: B=%d HW=%d D=%d", B, HW, D);
    const int64_t M = (int64_t)B * HW;
    hipLaunchKernelGGL(deeplab::assemble_fwd_kernel, dim3(deeplab::grid_for(M * 5 * D / 4)), dim3(256), 0, as_stream(stream), (const bf16*)a0,
                       (const bf16*)a1, (const bf16*)a2, (const bf16*)a3, pooled, (bf16*)buf, M, HW, D);
    P4C_CHECK_LAUNCH("p4c_deeplab_assemble_fwd");
    return P4C_OK;
}

extern "C" int p4c_deeplab_assemble_bwd(const void* dbuf, void* d0, void* d1, void* d2, void* d3, int B, int HW, int D, p4c_stream_t stream) {
    P4C_CHECK_ARG(dbuf && d0 && d1 && d2 && d3, "p4c_deeplab_assemble_bwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && HW > 0 && D > 0 && D % 4 == 0, "p4c_deeplab_assemble_bwd: B=%d HW=%d D=%d", B, HW, D);
    const int64_t M = (int64_t)B * HW;
    hipLaunchKernelGGL(deeplab::assemble_bwd_kernel, dim3(deeplab::grid_for(M * D)), dim3(256), 0, as_stream(stream), (const bf16*)dbuf, (bf16*)d0,
                       (bf16*)d1, (bf16*)d2, (bf16*)d3, M, D);
    P4C_CHECK_LAUNCH("p4c_deeplab_assemble_bwd");
    return P4C_OK;
}
