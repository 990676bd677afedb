// DeepLabV3+ (smp's DeepLabV3Plus on a torchvision ResNet encoder, as mfai builds it): the two passes that separate it from DeepLabV3 and
// that the GEMMs of csrc/gemm.hip, the batch-norm passes of csrc/inorm.hip and the ASPP passes of csrc/deeplab.hip do not cover.
// Features-last bf16 storage, fp32 arithmetic, every sum in a fixed order (no atomics): reruns and graph replays are bit-identical.  All
// are pure bandwidth: 16-byte (8-channel octet) loads and stores, no LDS on the element path, a grid-stride loop under a grid cap, int64
// pixel offsets.
//
//   dw3x3  : the depthwise half of the separable convolutions -- y_r = depthwise3x3(x; w_r, padding = dilation = d_r), no bias, for the
//            R <= 3 rates of the ASPP in ONE launch: a thread owns one octet of one pixel, loads the centre tap once for all rates and the
//            8 R others (1 + 8 R loads, not 9 R).  A tap outside the map is SKIPPED (zero padding), never clamped or wrapped, so d >= H
//            or d >= W degenerate to the taps that remain (the centre alone when both).  R = 1, d = 1: the undilated separable
//            convolutions.  Data gradient, one launch: dx[p] = sum_r sum_t w_r[t] dy_r[p - off_t] in fp32, r = 0 .. R-1 outermost, the
//            taps in row-major order, rounded once.  Weight gradient, one launch: per-chunk fp32 partials [rows][R][9][C] over x and the
//            R dy_r (a fixed-order reduction of the table follows: p4c_seg_reduce_partials).
//   upcat  : forward -- out (B, s h, s w, ld) = [bilinear_align_corners_xs(a) | skip | zeros up to ld] in ONE pass: no full-resolution
//            up-sampled map of its own, no concatenation copy.  The index, weight and blend arithmetic is resize_ac.hpp's, the same
//            statements p4c_upsample_bilinear_ac_fwd compiles: the up-sampled channels equal that kernel's bit for bit.  Backward -- one
//            pass over dout: da in gather form with the exact per-row check (resize_ac::gather8), dskip = the channel slice copied.
#include "common.hpp"
#include "resize_ac.hpp"

namespace p4c {
namespace dlp {

using resize_ac::pack8;
using resize_ac::u32x4;
using resize_ac::unpack8;

constexpr int GRID_CAP = 2048;        // 256 CUs x 8 workgroups of 256 threads: 524288 octets per trip, the loop strides over the rest
inline int grid_for(int64_t n) { return (int)((n + 255) / 256 < GRID_CAP ? (n + 255) / 256 : GRID_CAP); }
constexpr int MAX_RATES = 3;
constexpr int MAX_RATE = 4095;

struct Maps {                          // the R per-rate maps of a launch (y_r or dy_r) and their dilations
    bf16* m[MAX_RATES];
    int d[MAX_RATES];
};

__device__ __forceinline__ void load8(const bf16* p, float (&v)[8]) { unpack8(*reinterpret_cast<const u32x4*>(p), v); }
__device__ __forceinline__ void store8(bf16* p, const float (&v)[8]) { *reinterpret_cast<u32x4*>(p) = pack8(v); }
// the 8 fp32 weights of one tap of one channel octet (32 contiguous bytes of a [tap][C] row: coalesced across the octets of a wave)
__device__ __forceinline__ void loadw8(const float* p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// ---------------------------------------------------------------- depthwise 3x3, R rates
// unit = one octet of one pixel; w (R, 9, C) fp32: tap-major, so a tap's weights of an octet are one 32-byte load
template <int R>
__global__ void __launch_bounds__(256) dw_fwd_kernel(const bf16* __restrict__ x, const float* __restrict__ w, Maps y, int B, int H, int W, int C) {
    const int cg = C >> 3;
    const int64_t n = (int64_t)B * H * W * cg;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c0 = (int)(i % cg) * 8;
        const int64_t p = i / cg;
        const int px = (int)(p % W);
        const int64_t t = p / W;
        const int py = (int)(t % H);
        const int64_t b = t / H;
        float ctr[8];
        load8(x + p * C + c0, ctr);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float* wr = w + (int64_t)r * 9 * C + c0;
            const int d = y.d[r];
            float acc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                float wt[8];
                if (tap == 4) {
                    loadw8(wr + 4 * C, wt);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(wt[j], ctr[j], acc[j]);
                    continue;
                }
                const int sy = py + (tap / 3 - 1) * d, sx = px + (tap % 3 - 1) * d;
                if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
                float v[8];
                load8(x + ((b * H + sy) * W + sx) * C + c0, v);
                loadw8(wr + tap * C, wt);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(wt[j], v[j], acc[j]);
            }
            store8(y.m[r] + p * C + c0, acc);
        }
    }
}

// dx[p] = sum_r sum_t w_r[t] dy_r[p - off_t]: r outermost, taps in row-major order, one rounding
template <int R>
__global__ void __launch_bounds__(256) dw_dgrad_kernel(Maps dy, const float* __restrict__ w, bf16* __restrict__ dx, int B, int H, int W, int C) {
    const int cg = C >> 3;
    const int64_t n = (int64_t)B * H * W * cg;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c0 = (int)(i % cg) * 8;
        const int64_t p = i / cg;
        const int px = (int)(p % W);
        const int64_t t = p / W;
        const int py = (int)(t % H);
        const int64_t b = t / H;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float* wr = w + (int64_t)r * 9 * C + c0;
            const bf16* g = dy.m[r];
            const int d = dy.d[r];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int sy = py - (tap / 3 - 1) * d, sx = px - (tap % 3 - 1) * d;
                if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
                float v[8], wt[8];
                load8(g + ((b * H + sy) * W + sx) * C + c0, v);
                loadw8(wr + tap * C, wt);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(wt[j], v[j], acc[j]);
            }
        }
        store8(dx + p * C + c0, acc);
    }
}

// pixels per workgroup of the weight gradient: 4 waves of 16 (maps below 16384 pixels: the stride-16 maps, where the launch needs the
// workgroups) or of 32 pixels
inline int wgrad_block_pixels(int64_t P) { return P < 16384 ? 64 : 128; }

// grid (pixel chunks, channel-octet blocks of 64, R), block (64, 4): wave ty sums dy_r[p] x[p + off_t] over its quarter of the chunk's
// pixels in ascending order; the four waves' sums are added through LDS in the order 0, 1, 2, 3: partial[chunk][r][9][C]
__global__ void __launch_bounds__(256) dw_wgrad_kernel(const bf16* __restrict__ x, Maps dy, float* __restrict__ partial, int R, int B, int H, int W,
                                                       int C, int ppw) {
    __shared__ float red[3][64][9];                       // one tap of the waves 1 .. 3 (row padded to 9 words)
    const int lane = threadIdx.x, cgi = blockIdx.y * 64 + lane, ty = threadIdx.y, r = blockIdx.z;
    const bool active = cgi * 8 < C;
    const int c0 = active ? cgi * 8 : 0;
    const int64_t P = (int64_t)B * H * W;
    const bf16* g0 = r == 0 ? dy.m[0] : r == 1 ? dy.m[1] : dy.m[2];
    const int d = r == 0 ? dy.d[0] : r == 1 ? dy.d[1] : dy.d[2];
    float aw[9][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int t = 0; t < 9; ++t) aw[t][j] = 0.f;
    }
    const int64_t p0 = ((int64_t)blockIdx.x * 4 + ty) * ppw;
    for (int q = 0; q < ppw && active; ++q) {
        const int64_t p = p0 + q;
        if (p >= P) break;
        const int px = (int)(p % W);
        const int64_t t = p / W;
        const int py = (int)(t % H);
        const int64_t b = t / H;
        float g[8];
        load8(g0 + p * C + c0, g);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int sy = py + (tap / 3 - 1) * d, sx = px + (tap % 3 - 1) * d;
            if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
            float v[8];
            load8(x + ((b * H + sy) * W + sx) * C + c0, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) aw[tap][j] = __builtin_fmaf(g[j], v[j], aw[tap][j]);
        }
    }
    float* out = partial + ((int64_t)blockIdx.x * R + r) * (int64_t)(9 * C) + c0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        if (ty > 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) red[ty - 1][lane][j] = aw[t][j];
        }
        __syncthreads();
        if (ty == 0 && active) {
            float4 lo, hi;
            float sum[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) sum[j] = ((aw[t][j] + red[0][lane][j]) + red[1][lane][j]) + red[2][lane][j];
            lo.x = sum[0]; lo.y = sum[1]; lo.z = sum[2]; lo.w = sum[3];
            hi.x = sum[4]; hi.y = sum[5]; hi.z = sum[6]; hi.w = sum[7];
            *reinterpret_cast<float4*>(out + t * C) = lo;
            *reinterpret_cast<float4*>(out + t * C + 4) = hi;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- bilinear (align_corners) x scale + concatenation
// unit = one octet of one OUTPUT pixel's ld-wide row: octets [0, oa8) are up-sampled from a, [oa8, oa8 + os8) copied from skip, the rest
// (ld > Ca + Cs) written as zeros
__global__ void __launch_bounds__(256) upcat_fwd_kernel(const bf16* __restrict__ a, const bf16* __restrict__ skip, bf16* __restrict__ out, int64_t ld,
                                                        int B, int h, int w, int Ca, int Cs, int scale) {
    const int OH = h * scale, OW = w * scale;
    const int oa8 = Ca >> 3, os8 = Cs >> 3, per = (int)(ld >> 3);
    const float sy = resize_ac::ac_scale(h, OH), sx = resize_ac::ac_scale(w, OW);
    const int64_t n = (int64_t)B * OH * OW * per;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int o = (int)(g % per);
        const int64_t pix = g / per;
        bf16* dst = out + pix * ld + o * 8;
        if (o < oa8) {
            const int ox = (int)(pix % OW);
            const int64_t t = pix / OW;
            const int oy = (int)(t % OH);
            const int64_t b = t / OH;
            int y0, y1, x0, x1;
            float ly, lx;
            resize_ac::src_index_ac(oy, sy, h, y0, y1, ly);
            resize_ac::src_index_ac(ox, sx, w, x0, x1, lx);
            float v[8];
            resize_ac::blend8(a + b * h * w * Ca + 8 * o, w, Ca, y0, y1, x0, x1, ly, lx, v);
            store8(dst, v);
        } else if (o < oa8 + os8) {
            *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(skip + pix * Cs + (o - oa8) * 8);
        } else {
            const u32x4 z = {0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(dst) = z;
        }
    }
}

// units [0, na): one octet of one pixel of da (gather over dout's first Ca channels); [na, na + ns): one octet of one pixel of dskip
__global__ void __launch_bounds__(256) upcat_bwd_kernel(const bf16* __restrict__ dout, int64_t ld, bf16* __restrict__ da, bf16* __restrict__ dskip,
                                                        int B, int h, int w, int Ca, int Cs, int scale) {
    const int OH = h * scale, OW = w * scale;
    const int oa8 = Ca >> 3, os8 = Cs >> 3;
    const float sy = resize_ac::ac_scale(h, OH), sx = resize_ac::ac_scale(w, OW);
    const int64_t na = (int64_t)B * h * w * oa8, ns = (int64_t)B * OH * OW * os8;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < na + ns; g += (int64_t)gridDim.x * 256) {
        if (g < na) {
            const int q = (int)(g % oa8);
            const int64_t p = g / oa8;
            const int ix = (int)(p % w);
            const int64_t t = p / w;
            const int iy = (int)(t % h);
            const int64_t b = t / h;
            float acc[8];
            resize_ac::gather8(dout + b * OH * OW * ld + 8 * q, ld, iy, ix, h, w, OH, OW, sy, sx, acc);
            store8(da + p * Ca + 8 * q, acc);
        } else {
            const int64_t e = g - na;
            const int q = (int)(e % os8);
            const int64_t pix = e / os8;
            *reinterpret_cast<u32x4*>(dskip + pix * Cs + 8 * q) = *reinterpret_cast<const u32x4*>(dout + pix * ld + Ca + 8 * q);
        }
    }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// argument checks shared by the three depthwise entry points; fills `m`
static int dw_maps(const char* name, void* const* maps, const int* rates, int R, int B, int H, int W, int C, Maps& m) {
    P4C_CHECK_ARG(R >= 1 && R <= MAX_RATES, "%s: R=%d (1 .. %d rates)", name, R, MAX_RATES);
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && H <= (1 << 20) && W <= (1 << 20) && C > 0 && C % 8 == 0, "%s: B=%d H=%d W=%d C=%d (C a multiple of 8)",
                  name, B, H, W, C);
    for (int r = 0; r < MAX_RATES; ++r) {
        m.m[r] = nullptr;
        m.d[r] = 1;
    }
    for (int r = 0; r < R; ++r) {
        P4C_CHECK_ARG(maps[r] && aligned16(maps[r]), "%s: map %d is NULL or not 16-byte aligned", name, r);
        P4C_CHECK_ARG(rates[r] >= 1 && rates[r] <= MAX_RATE, "%s: rate %d = %d (1 .. %d)", name, r, rates[r], MAX_RATE);
        m.m[r] = (bf16*)maps[r];
        m.d[r] = rates[r];
    }
    return P4C_OK;
}

}  // namespace dlp
}  // namespace p4c

using namespace p4c;

extern "C" int p4c_dlp_dw3x3_fwd(const void* x, const float* w, void* y0, void* y1, void* y2, int R, int d0, int d1, int d2, int B, int H, int W,
                                 int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(x && w && dlp::aligned16(x) && dlp::aligned16(w), "p4c_dlp_dw3x3_fwd: x or w is NULL or not 16-byte aligned");
    void* const maps[3] = {y0, y1, y2};
    const int rates[3] = {d0, d1, d2};
    dlp::Maps m;
    P4C_TRY(dlp::dw_maps("p4c_dlp_dw3x3_fwd", maps, rates, R, B, H, W, C, m));
    const int64_t n = (int64_t)B * H * W * (C / 8);
    const dim3 grid(dlp::grid_for(n)), block(256);
    hipStream_t st = as_stream(stream);
    if (R == 1) hipLaunchKernelGGL(dlp::dw_fwd_kernel<1>, grid, block, 0, st, (const bf16*)x, w, m, B, H, W, C);
    else if (R == 2) hipLaunchKernelGGL(dlp::dw_fwd_kernel<2>, grid, block, 0, st, (const bf16*)x, w, m, B, H, W, C);
    else hipLaunchKernelGGL(dlp::dw_fwd_kernel<3>, grid, block, 0, st, (const bf16*)x, w, m, B, H, W, C);
    P4C_CHECK_LAUNCH("p4c_dlp_dw3x3_fwd");
    return P4C_OK;
}

extern "C" int p4c_dlp_dw3x3_dgrad(const void* dy0, const void* dy1, const void* dy2, const float* w, void* dx, int R, int d0, int d1, int d2, int B,
                                   int H, int W, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(dx && w && dlp::aligned16(dx) && dlp::aligned16(w), "p4c_dlp_dw3x3_dgrad: dx or w is NULL or not 16-byte aligned");
    void* const maps[3] = {const_cast<void*>(dy0), const_cast<void*>(dy1), const_cast<void*>(dy2)};
    const int rates[3] = {d0, d1, d2};
    dlp::Maps m;
    P4C_TRY(dlp::dw_maps("p4c_dlp_dw3x3_dgrad", maps, rates, R, B, H, W, C, m));
    const int64_t n = (int64_t)B * H * W * (C / 8);
    const dim3 grid(dlp::grid_for(n)), block(256);
    hipStream_t st = as_stream(stream);
    if (R == 1) hipLaunchKernelGGL(dlp::dw_dgrad_kernel<1>, grid, block, 0, st, m, w, (bf16*)dx, B, H, W, C);
    else if (R == 2) hipLaunchKernelGGL(dlp::dw_dgrad_kernel<2>, grid, block, 0, st, m, w, (bf16*)dx, B, H, W, C);
    else hipLaunchKernelGGL(dlp::dw_dgrad_kernel<3>, grid, block, 0, st, m, w, (bf16*)dx, B, H, W, C);
    P4C_CHECK_LAUNCH("p4c_dlp_dw3x3_dgrad");
    return P4C_OK;
}

extern "C" int p4c_dlp_dw3x3_wgrad_rows(int B, int H, int W) {
    const int64_t P = (int64_t)B * H * W;
    if (P <= 0) return 0;
    const int pix = dlp::wgrad_block_pixels(P);
    return (int)((P + pix - 1) / pix);
}

extern "C" int p4c_dlp_dw3x3_wgrad(const void* x, const void* dy0, const void* dy1, const void* dy2, float* partial, int R, int d0, int d1, int d2,
                                   int B, int H, int W, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(x && partial && dlp::aligned16(x) && dlp::aligned16(partial), "p4c_dlp_dw3x3_wgrad: x or partial is NULL or not 16-byte aligned");
    void* const maps[3] = {const_cast<void*>(dy0), const_cast<void*>(dy1), const_cast<void*>(dy2)};
    const int rates[3] = {d0, d1, d2};
    dlp::Maps m;
    P4C_TRY(dlp::dw_maps("p4c_dlp_dw3x3_wgrad", maps, rates, R, B, H, W, C, m));
    P4C_CHECK_ARG((int64_t)B * H * W <= (1LL << 30), "p4c_dlp_dw3x3_wgrad: B H W beyond 2^30 pixels");
    const int rows = p4c_dlp_dw3x3_wgrad_rows(B, H, W);
    hipLaunchKernelGGL(dlp::dw_wgrad_kernel, dim3(rows, (C / 8 + 63) / 64, R), dim3(64, 4), 0, as_stream(stream), (const bf16*)x, m, partial, R, B,
                       H, W, C, dlp::wgrad_block_pixels((int64_t)B * H * W) / 4);
    P4C_CHECK_LAUNCH("p4c_dlp_dw3x3_wgrad");
    return P4C_OK;
}

static int upcat_check(const char* name, int64_t ld, int B, int h, int w, int Ca, int Cs, int scale) {
    P4C_CHECK_ARG(B > 0 && h > 0 && w > 0 && h <= (1 << 16) && w <= (1 << 16) && scale >= 1 && scale <= 8, "%s: B=%d h=%d w=%d scale=%d (scale 1 .. 8)",
                  name, B, h, w, scale);
    P4C_CHECK_ARG(Ca > 0 && Ca % 8 == 0 && Cs > 0 && Cs % 8 == 0 && ld >= (int64_t)Ca + Cs && ld % 8 == 0 && ld <= (1 << 20),
                  "%s: Ca=%d Cs=%d ld=%lld (Ca, Cs, ld positive multiples of 8, ld >= Ca + Cs)", name, Ca, Cs, (long long)ld);
    return P4C_OK;
}

extern "C" int p4c_dlp_up_cat_fwd(const void* a, const void* skip, void* out, int64_t ld, int B, int h, int w, int Ca, int Cs, int scale,
                                  p4c_stream_t stream) {
    P4C_CHECK_ARG(a && skip && out, "p4c_dlp_up_cat_fwd: NULL pointer");
    P4C_TRY(upcat_check("p4c_dlp_up_cat_fwd", ld, B, h, w, Ca, Cs, scale));
    P4C_CHECK_ARG(dlp::aligned16(a) && dlp::aligned16(skip) && dlp::aligned16(out), "p4c_dlp_up_cat_fwd: operands must be 16-byte aligned");
    const int64_t n = (int64_t)B * h * scale * w * scale * (ld / 8);
    hipLaunchKernelGGL(dlp::upcat_fwd_kernel, dim3(dlp::grid_for(n)), dim3(256), 0, as_stream(stream), (const bf16*)a, (const bf16*)skip, (bf16*)out,
                       ld, B, h, w, Ca, Cs, scale);
    P4C_CHECK_LAUNCH("p4c_dlp_up_cat_fwd");
    return P4C_OK;
}

extern "C" int p4c_dlp_up_cat_bwd(const void* dout, int64_t ld, void* da, void* dskip, int B, int h, int w, int Ca, int Cs, int scale,
                                  p4c_stream_t stream) {
    P4C_CHECK_ARG(dout && da && dskip, "p4c_dlp_up_cat_bwd: NULL pointer");
    P4C_TRY(upcat_check("p4c_dlp_up_cat_bwd", ld, B, h, w, Ca, Cs, scale));
    P4C_CHECK_ARG(dlp::aligned16(dout) && dlp::aligned16(da) && dlp::aligned16(dskip), "p4c_dlp_up_cat_bwd: operands must be 16-byte aligned");
    const int64_t n = (int64_t)B * h * w * (Ca / 8) + (int64_t)B * h * scale * w * scale * (Cs / 8);
    hipLaunchKernelGGL(dlp::upcat_bwd_kernel, dim3(dlp::grid_for(n)), dim3(256), 0, as_stream(stream), (const bf16*)dout, ld, (bf16*)da, (bf16*)dskip,
                       B, h, w, Ca, Cs, scale);
    P4C_CHECK_LAUNCH("p4c_dlp_up_cat_bwd");
    return P4C_OK;
}
