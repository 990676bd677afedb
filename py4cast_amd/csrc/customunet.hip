// CustomUNet (smp's Unet on a torchvision ResNet encoder, as mfai builds it): the two decoder-side passes that the GEMMs of csrc/gemm.hip
// and the batch-norm passes of csrc/inorm.hip do not cover.  Features-last bf16 storage, fp32 arithmetic, every sum in a fixed order (no
// atomics): reruns and graph replays are bit-identical.  Both are pure bandwidth: no LDS on the element path, a grid-stride loop.
//
//   up2cat    : forward -- out (B, 2h, 2w, ld) = [nearest_x2(x) | skip]: out[b][2i+di][2j+dj][0:Cx] = x[b][i][j][:] and
//               out[..][Cx:Cx+Cs] = skip[b][2i+di][2j+dj][:], in ONE pass (F.interpolate + torch.cat: three full-resolution passes).  A
//               thread moves 8 channels (16 bytes) of the 2x2 output block of one input pixel: an x octet is loaded once and stored four
//               times.  skip == NULL: the channels from Cx on are left as their producer wrote them (the stem tail below).
//               Backward -- one pass over dout: dx[b][i][j][c] = the four dout[b][2i+di][2j+dj][c] added in fp32 in the order (0,0), (0,1),
//               (1,0), (1,1), rounded once; dskip = the channel slice copied (dskip == NULL: its consumer reads dout in place).
//   stem tail : p4c_deeplab_stem_fwd / _bwd with one more output -- the kernels of csrc/stem_tail.hpp WITH their skip: act = relu(y scale
//               + shift), rounded to bf16, goes to the concatenation buffer of decoder block 3 (pointer + row stride, as
//               p4c_unet_enc_tail_fwd writes its skip) in the same pass that pools it.  Backward: dz = relu'(act) (dskip + the dpool of
//               the windows that chose this pixel, in window order).  Same tie rule: the window's first maximum in row-major order.
#include "common.hpp"
#include "stem_tail.hpp"

namespace p4c {
namespace customunet {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int GRID_CAP = 2048;        // 256 CUs x 8 workgroups; the loop strides over the rest
inline int grid_for(int64_t n) { return (int)((n + 255) / 256 < GRID_CAP ? (n + 255) / 256 : GRID_CAP); }

// ---------------------------------------------------------------- nearest x2 + concatenation
// unit = one 8-channel octet of one INPUT pixel's 2x2 output block; octets [0, ox8) come from x, [ox8, ox8 + os8) from skip
__global__ void __launch_bounds__(256) up2cat_fwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ skip, bf16* __restrict__ out, int64_t ld,
                                                         int B, int h, int w, int Cx, int Cs) {
    const int ox8 = Cx >> 3, os8 = skip ? Cs >> 3 : 0, per = ox8 + os8;
    const int64_t n = (int64_t)B * h * w * per;
    const int W2 = 2 * w;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int o = (int)(g % per);
        const int64_t pix = g / per;
        const int j = (int)(pix % w);
        const int64_t t = pix / w;
        const int i = (int)(t % h);
        const int64_t b = t / h;
        const int64_t r0 = (b * 2 * h + 2 * i) * W2 + 2 * j;       // output pixel (2i, 2j)
        if (o < ox8) {
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + pix * Cx + o * 8);
            bf16* d = out + r0 * ld + o * 8;
            *reinterpret_cast<bf16x8*>(d) = v;
            *reinterpret_cast<bf16x8*>(d + ld) = v;
            *reinterpret_cast<bf16x8*>(d + W2 * ld) = v;
            *reinterpret_cast<bf16x8*>(d + (W2 + 1) * ld) = v;
        } else {
            const int c = (o - ox8) * 8;
            const bf16* s = skip + r0 * Cs + c;
            bf16* d = out + r0 * ld + Cx + c;
            const bf16x8 v0 = *reinterpret_cast<const bf16x8*>(s), v1 = *reinterpret_cast<const bf16x8*>(s + Cs);
            const bf16x8 v2 = *reinterpret_cast<const bf16x8*>(s + (int64_t)W2 * Cs), v3 = *reinterpret_cast<const bf16x8*>(s + (int64_t)(W2 + 1) * Cs);
            *reinterpret_cast<bf16x8*>(d) = v0;
            *reinterpret_cast<bf16x8*>(d + ld) = v1;
            *reinterpret_cast<bf16x8*>(d + W2 * ld) = v2;
            *reinterpret_cast<bf16x8*>(d + (W2 + 1) * ld) = v3;
        }
    }
}

__global__ void __launch_bounds__(256) up2cat_bwd_kernel(const bf16* __restrict__ dout, int64_t ld, bf16* __restrict__ dx, bf16* __restrict__ dskip,
                                                         int B, int h, int w, int Cx, int Cs) {
    const int ox8 = Cx >> 3, os8 = dskip ? Cs >> 3 : 0, per = ox8 + os8;
    const int64_t n = (int64_t)B * h * w * per;
    const int W2 = 2 * w;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int o = (int)(g % per);
        const int64_t pix = g / per;
        const int j = (int)(pix % w);
        const int64_t t = pix / w;
        const int i = (int)(t % h);
        const int64_t b = t / h;
        const int64_t r0 = (b * 2 * h + 2 * i) * W2 + 2 * j;
        const bf16* s = dout + r0 * ld + o * 8;                    // (o >= ox8: channel Cx + (o - ox8) 8 = o 8)
        const bf16x8 v0 = *reinterpret_cast<const bf16x8*>(s), v1 = *reinterpret_cast<const bf16x8*>(s + ld);
        const bf16x8 v2 = *reinterpret_cast<const bf16x8*>(s + W2 * ld), v3 = *reinterpret_cast<const bf16x8*>(s + (W2 + 1) * ld);
        if (o < ox8) {
            bf16x8 r;
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = (__bf16)((((float)v0[e] + (float)v1[e]) + (float)v2[e]) + (float)v3[e]);
            *reinterpret_cast<bf16x8*>(dx + pix * Cx + o * 8) = r;
        } else {
            bf16* d = dskip + r0 * Cs + (o - ox8) * 8;
            *reinterpret_cast<bf16x8*>(d) = v0;
            *reinterpret_cast<bf16x8*>(d + Cs) = v1;
            *reinterpret_cast<bf16x8*>(d + (int64_t)W2 * Cs) = v2;
            *reinterpret_cast<bf16x8*>(d + (int64_t)(W2 + 1) * Cs) = v3;
        }
    }
}

}  // namespace customunet
}  // namespace p4c

using namespace p4c;

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

extern "C" int p4c_up2_cat_fwd(const void* x, const void* skip, void* out, int64_t ld, int B, int h, int w, int Cx, int Cs, p4c_stream_t stream) {
    P4C_CHECK_ARG(x && out, "p4c_up2_cat_fwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && h > 0 && w > 0 && h <= (1 << 20) && w <= (1 << 20) && Cx > 0 && Cx % 8 == 0 && Cs >= 0 && Cs % 8 == 0
                  && ld >= (int64_t)Cx + Cs && ld % 8 == 0 && (Cs > 0 || !skip),
                  "p4c_up2_cat_fwd: B=%d h=%d w=%d Cx=%d Cs=%d ld=%lld (Cx, Cs, ld multiples of 8, ld >= Cx + Cs)", B, h, w, Cx, Cs, (long long)ld);
    P4C_CHECK_ARG(aligned16(x) && aligned16(skip) && aligned16(out), "p4c_up2_cat_fwd: operands must be 16-byte aligned");
    const int64_t n = (int64_t)B * h * w * ((Cx + (skip ? Cs : 0)) / 8);
    hipLaunchKernelGGL(customunet::up2cat_fwd_kernel, dim3(customunet::grid_for(n)), dim3(256), 0, as_stream(stream), (const bf16*)x,
                       (const bf16*)skip, (bf16*)out, ld, B, h, w, Cx, Cs);
    P4C_CHECK_LAUNCH("p4c_up2_cat_fwd");
    return P4C_OK;
}

extern "C" int p4c_up2_cat_bwd(const void* dout, int64_t ld, void* dx, void* dskip, int B, int h, int w, int Cx, int Cs, p4c_stream_t stream) {
    P4C_CHECK_ARG(dout && dx, "p4c_up2_cat_bwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && h > 0 && w > 0 && h <= (1 << 20) && w <= (1 << 20) && Cx > 0 && Cx % 8 == 0 && Cs >= 0 && Cs % 8 == 0
                  && ld >= (int64_t)Cx + Cs && ld % 8 == 0 && (Cs > 0 || !dskip),
                  "p4c_up2_cat_bwd: B=%d h=%d w=%d Cx=%d Cs=%d ld=%lld (Cx, Cs, ld multiples of 8, ld >= Cx + Cs)", B, h, w, Cx, Cs, (long long)ld);
    P4C_CHECK_ARG(aligned16(dout) && aligned16(dx) && aligned16(dskip), "p4c_up2_cat_bwd: operands must be 16-byte aligned");
    const int64_t n = (int64_t)B * h * w * ((Cx + (dskip ? Cs : 0)) / 8);
    hipLaunchKernelGGL(customunet::up2cat_bwd_kernel, dim3(customunet::grid_for(n)), dim3(256), 0, as_stream(stream), (const bf16*)dout, ld,
                       (bf16*)dx, (bf16*)dskip, B, h, w, Cx, Cs);
    P4C_CHECK_LAUNCH("p4c_up2_cat_bwd");
    return P4C_OK;
}

extern "C" int p4c_customunet_stem_fwd(const void* y, const float* scale, const float* shift, void* skip, int64_t ld, void* pool, void* arg, int B,
                                       int H, int W, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(y && scale && shift && skip && pool && arg, "p4c_customunet_stem_fwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && C <= 1024 && ld >= C && ld % 4 == 0 && aligned8(skip),
                  "p4c_customunet_stem_fwd: B=%d H=%d W=%d C=%d ld=%lld (C a multiple of 4 up to 1024, ld >= C a multiple of 4, skip 8-byte "
                  "aligned)", B, H, W, C, (long long)ld);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t n = (int64_t)B * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(stem::tail_fwd_kernel<true>, dim3(customunet::grid_for(n)), dim3(256), 0, as_stream(stream), (const bf16*)y, scale, shift,
                       (bf16*)skip, ld, (bf16*)pool, (unsigned char*)arg, B, H, W, C, Ho, Wo);
    P4C_CHECK_LAUNCH("p4c_customunet_stem_fwd");
    return P4C_OK;
}

extern "C" int p4c_customunet_stem_bwd_blocks(int B, int H, int W, int C) { return stem::bwd_blocks(B, H, W, C); }

extern "C" int p4c_customunet_stem_bwd(const void* y, const void* dskip, int64_t ld, const void* dpool, const void* arg, const float* scale,
                                       const float* shift, const float* mean, const float* rstd, void* dz, float* partial, int B, int H, int W,
                                       int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(y && dskip && dpool && arg && scale && shift && mean && rstd && dz && partial, "p4c_customunet_stem_bwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && C <= 1024 && ld >= C && ld % 4 == 0 && aligned8(dskip),
                  "p4c_customunet_stem_bwd: B=%d H=%d W=%d C=%d ld=%lld", B, H, W, C, (long long)ld);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int nb = stem::bwd_blocks(B, H, W, C);
    const size_t smem = (size_t)stem::bwd_pixels_per_block(C) * 2 * C * sizeof(float);
    hipLaunchKernelGGL(stem::tail_bwd_kernel<true>, dim3(nb), dim3(256), smem, as_stream(stream), (const bf16*)y, (const bf16*)dskip, ld,
                       (const bf16*)dpool, (const unsigned char*)arg, scale, shift, mean, rstd, (bf16*)dz, partial, B, H, W, C, Ho, Wo);
    P4C_CHECK_LAUNCH("p4c_customunet_stem_bwd");
    return P4C_OK;
}
