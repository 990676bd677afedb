// The first convolution of the HalfUNet plan at the benchmark's 69 input channels (60 state + 5 forcing + 4 static features:
// py4cast/lightning.py:256-261, 711-767), as TWO launches instead of one generic K = 96 launch (round 6; bf16 flavour only):
//
//   1. the row-streaming kernel of conv_rows.hip on input channels 0..63 (a 64 -> 64 launch like every other convolution of the
//      network, reading the 96-channel pixels of x with a 192-byte stride): y1 = conv3x3(x[..., :64]);
//   2. first_conv_tail_kernel (here): y = bf16(y1 + conv3x3(x[..., 64:72])) and the BatchNorm / GroupNorm sums of y -- an HBM-bound
//      pass over y (read + write) that carries the 5 channels beyond 64 as a K = 80 product per 32 pixels (9 taps x 8 channels + one
//      zero tap): 10 v_mfma_f32_32x32x16_bf16 per 32 pixels x 64 output channels against 108 for a 96-channel launch.
//
// The generic role-split kernel it replaces (conv_fwd_bf16_kernel<96, 3>) took 91-100 us per launch x 3 AR steps for 1.5 x the matrix
// work of a 64-channel launch that takes 39-43.  Numerics: y1 is rounded to bf16 before the tail adds its fp32 product
// -- a second rounding that the one-launch form does not have; inside every bar the bf16 flavour is held to (the fp32 flavour keeps the
// one-launch kernel).  Since then the plan runs the convolution as ONE launch of the row kernel that carries the octet beyond 64 itself
// (conv_rows.hip: THIN; first_conv_one_routed below) -- this two-launch form stays as the route of P4C_FIRST_CONV_ONE=0 (diagnostic
// build), as the reference of the parity tests and behind p4c_first_conv_tail / p4c_first_conv_two.  The backward: data gradient = a
// 64 -> 64 row launch on the state channels; weight gradient = the row-streaming kernel's full chunk + conv3x3_wgrad_thin_bf16_kernel (below) for the rows of the channels beyond 64.
#include <stdlib.h>

#include <atomic>

#include "kernels.hpp"

namespace p4c {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int OOB = 0x7fffffff;
constexpr int SP = 68;                   // floats per pixel of a wave's staging tile (64 + 4: 16-byte aligned rows off the bank period)
constexpr int WIMG_BYTES = 2 * 5 * 64 * 16;

struct ThinArgs {
    const __bf16* x;        // (B, H, W, x_cs) bf16
    const float* w;         // fp32 master weight [64][cin][3][3]
    __bf16* y;              // (B, H, W, 64): in = y1, out = y (in place: every element is read and written by one lane)
    float* stat_partial;    // [B][nblk * 4][2][64] sums / sums of squares of the stored y, or NULL
    int x_cs, c0, nc, cin;  // pixel stride of x in channels; first tail channel (64); tail channels (1..8); input channels of w
    int H, W, nblk;
};

__device__ __forceinline__ float bf_lo(unsigned int w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf_hi(unsigned int w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
__device__ __forceinline__ unsigned int pack2(float lo, float hi) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf16x2));
}

__global__ void __launch_bounds__(256) first_conv_tail_kernel(ThinArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[WIMG_BYTES + 4 * 32 * SP * 4];
    __bf16* wimg = reinterpret_cast<__bf16*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
    float* tile = reinterpret_cast<float*>(smem + WIMG_BYTES) + wv * 32 * SP;
    // A operands: image[(ct * 5 + s) * 64 + lane] = 8 bf16 = W[co = 32 ct + (lane & 31)][c0 + j][tap 2 s + (lane >> 5)], zero for the
    // tenth tap and the channels beyond the real ones
    for (int idx = tid; idx < 2 * 5 * 64; idx += 256) {
        const int l = idx & 63, ts = idx >> 6;
        const int s = ts % 5, ct = ts / 5;
        const int co = 32 * ct + (l & 31), tap = 2 * s + (l >> 5);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (__bf16)((tap < 9 && j < a.nc) ? a.w[((int64_t)co * a.cin + a.c0 + j) * 9 + tap] : 0.f);
        *reinterpret_cast<bf16x8*>(wimg + idx * 8) = o;
    }
    __syncthreads();
    bf16x8 A[2][5];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int s = 0; s < 5; ++s) A[ct][s] = *reinterpret_cast<const bf16x8*>(wimg + ((ct * 5 + s) * 64 + lane) * 8);

    const int b = blockIdx.y, H = a.H, W = a.W;
    const int64_t npix = (int64_t)H * W;
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(a.x + (int64_t)b * npix * a.x_cs), 0,
                                                                        (int)(npix * a.x_cs * 2), 0x00020000);
    __bf16* yb = a.y + (int64_t)b * npix * 64;
    const int ngroups = (int)(npix / 32);            // W % 32 == 0 (host): a group of 32 pixels lies in one image row
    const int wid = blockIdx.x * 4 + wv, nwaves = a.nblk * 4;
    const int prow = lane >> 3, c8 = lane & 7;       // row layout: pixel 8 it + prow of the group, channels 8 c8 .. +7
    float a1[8], a2[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) a1[q] = a2[q] = 0.f;

    // the NEXT group's operands (5 tap octets + 4 row pieces of y per lane) are in flight while the current group is multiplied, transposed
    // and stored: a wave walks ~8 groups, and without the prefetch every one of them exposed its full memory round trip (45-51 us per
    // launch for 134 MB in the first trace of the round)
    auto load_group = [&](int g, bf16x8 (&bop)[5], u32x4 (&yq)[4]) __attribute__((always_inline)) {
        const bool live = g < ngroups;
        const int p0 = live ? g * 32 : 0, yy = p0 / W, x0 = p0 - yy * W;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const int tap = 2 * s + h, dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
            const int sy = yy + dy, sx = x0 + r + dx;
            const bool ok = live && tap < 9 && (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W;
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_x, ok ? ((sy * W + sx) * a.x_cs + a.c0) * 2 : OOB, 0, 0);
            bop[s] = __builtin_bit_cast(bf16x8, v);
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) yq[it] = *reinterpret_cast<const u32x4*>(yb + ((int64_t)p0 + 8 * it + prow) * 64 + 8 * c8);
    };
    bf16x8 Bop[5], Bnx[5];
    u32x4 yv[4], ynx[4];
    load_group(wid, Bop, yv);
    for (int g = wid; g < ngroups; g += nwaves) {
        const int p0 = g * 32;
        load_group(g + nwaves, Bnx, ynx);
        f32x16 acc[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[ct][i] = 0.f;
#pragma unroll
            for (int s = 0; s < 5; ++s) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[ct][s], Bop[s], acc[ct], 0, 0, 0);
        }
        // accumulator layout (lane = pixel r, registers 4 q + e = channels 32 ct + 8 q + 4 h + e) -> the wave's [pixel][channel] tile
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<f32x4*>(tile + r * SP + 32 * ct + 8 * q + 4 * h) = f32x4{acc[ct][4 * q], acc[ct][4 * q + 1], acc[ct][4 * q + 2], acc[ct][4 * q + 3]};
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int px = 8 * it + prow;
            const f32x4 t0 = *reinterpret_cast<const f32x4*>(tile + px * SP + 8 * c8), t1 = *reinterpret_cast<const f32x4*>(tile + px * SP + 8 * c8 + 4);
            const float t[8] = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
            u32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o[k] = pack2(bf_lo(yv[it][k]) + t[2 * k], bf_hi(yv[it][k]) + t[2 * k + 1]);
                const float lo = bf_lo(o[k]), hi = bf_hi(o[k]);       // statistics of the STORED values
                a1[2 * k] += lo; a2[2 * k] = __builtin_fmaf(lo, lo, a2[2 * k]);
                a1[2 * k + 1] += hi; a2[2 * k + 1] = __builtin_fmaf(hi, hi, a2[2 * k + 1]);
            }
            *reinterpret_cast<u32x4*>(yb + ((int64_t)p0 + px) * 64 + 8 * c8) = o;
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
#pragma unroll
        for (int s = 0; s < 5; ++s) Bop[s] = Bnx[s];
#pragma unroll
        for (int it = 0; it < 4; ++it) yv[it] = ynx[it];
    }
    if (a.stat_partial) {
        // one [2][64] slot per wave (also from a wave without a group: the finalize sums every slot)
        float* dst = a.stat_partial + ((int64_t)b * nwaves + wid) * 128;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float u = a1[q], v = a2[q];
            u += __shfl_xor(u, 8); v += __shfl_xor(v, 8);
            u += __shfl_xor(u, 16); v += __shfl_xor(v, 16);
            u += __shfl_xor(u, 32); v += __shfl_xor(v, 32);
            if (lane < 8) { dst[8 * c8 + q] = u; dst[64 + 8 * c8 + q] = v; }
        }
    }
}

int tail_blocks(int B, int H, int W) {
    const int64_t groups = (int64_t)H * W / 32;
    int64_t n = (groups + 3) / 4;
    if (n > 256) n = 256;              // <= 1024 statistics slots per sample (the plan's statistics buffer holds >= 4 x CUs)
    const int64_t cap = 2 * (int64_t)num_cus() / (B > 0 ? B : 1);
    if (n > cap && cap >= 1) n = cap;
    return n < 1 ? 1 : (int)n;
}

}  // namespace

bool first_conv_split_ok(int compute, int storage, int cin, int cin_pad, int B, int H, int W) {
    const char* e = diag_env("P4C_FIRST_CONV_SPLIT");       // (A/B switch of the diagnostic build: 0 = the one-launch K = 96 kernel)
    if (e && e[0] == '0') return false;
    return compute == P4C_BF16 && storage == P4C_BF16 && cin_pad == 96 && cin > 64 && cin <= 72 && W % 32 == 0 &&
           conv_bf16_is_rows(storage, 64, 3, 1, 64, B, H, W) && (int64_t)H * W * 192 < ((int64_t)1 << 31);
}

// ... and of those shapes, the ones the plan runs as ONE launch of the row kernel (conv_rows.hip: THIN) instead of row launch + tail
bool first_conv_one_routed(int compute, int storage, int cin, int cin_pad, int B, int H, int W) {
    const char* e = diag_env("P4C_FIRST_CONV_ONE");         // (A/B switch of the diagnostic build: 0 = row launch + tail)
    if (e && e[0] == '0') return false;
    return first_conv_split_ok(compute, storage, cin, cin_pad, B, H, W) && first_conv_one_ok(cin_pad, B, H, W);
}

int first_conv_tail_slots(int B, int H, int W) { return tail_blocks(B, H, W) * 4; }

// kernels this process has enqueued for the first convolution at 65..72 input channels, counted where they are launched (the
// one-launch row kernel, the row launch on wide pixels, the tail): p4c_first_conv_launch_count, what the route test asserts on
static std::atomic<long long> g_first_conv_launches{0};
void count_first_conv_launch() { g_first_conv_launches.fetch_add(1); }
long long first_conv_launches() { return g_first_conv_launches.load(); }

int launch_first_conv_tail(const void* x, int x_cs, int cin, const float* w, void* y, float* stat_partial, int B, int H, int W, hipStream_t stream) {
    ThinArgs a{(const __bf16*)x, w, (__bf16*)y, stat_partial, x_cs, 64, cin - 64, cin, H, W, tail_blocks(B, H, W)};
    hipLaunchKernelGGL(first_conv_tail_kernel, dim3(a.nblk, B), dim3(256), 0, stream, a);
    count_first_conv_launch();
    P4C_CHECK_LAUNCH("first_conv_tail");
    return P4C_OK;
}

// ---------------------------------------------------------------------------------------------
// conv3x3_wgrad_thin_bf16: the weight gradient of the same convolution's channels beyond 64 (one octet: rows 64..71 of dW), the job the
// row-streaming kernel of conv_wgrad_rows.hip ran as a THIN chunk -- a second full launch (whole-CU workgroups, 66-pixel rows of a
// 32-channel tile that is seven-eighths zero, 9 tap tiles per wave, a slab sized for a full tile) for 5/64 of the result:
//
//   dW[ky][kx][64 + c][co] = sum over pixels of X[y + ky - 1][x + kx - 1][64 + c] * dY[y][x][co],  c = 0..7
//
// a GEMM with K = pixels, M = 9 taps x 8 channels = 72 (three 32-row tiles: 12 tap slots, the last three unused), N = 64.
//   * work item = a row segment of a 64-column strip of one sample (the geometry of the row-streaming kernels); persistent workgroups
//     walk items wg, wg + G, ... and keep their accumulators over all of them: ONE fp32 partial [9][8][64] (18 KB) per workgroup;
//   * 256 threads, every wave loads and multiplies.  An interval is two dY rows (2 x 64 px x 128 B, 16-byte coalesced loads into the
//     swizzled pixel layout of conv_wgrad_rows.hip) and two rows of x octets (66 px x 16 B, one 16-byte load per 192-byte pixel); the
//     next interval's loads are in flight in registers while the current one is multiplied, one workgroup barrier per interval.
//     An x row is loaded once for the three dY rows it meets (ring of 8 rows); the tap shift is an address offset into the octet
//     image, so each octet is read from memory once for its nine taps;
//   * wave = (32 output channels, one half of the 64 pixels) x 3 tap tiles = 48 accumulator registers; both operands by transposed
//     LDS reads; 6 MFMAs per 16 pixels and workgroup.  The two pixel halves are added in a fixed order at the end (LDS).
// LDS 41 KB, so several workgroups share a CU: a streaming job beside the backward chain (HBM: dY once + the octets).
namespace {
namespace wt {
constexpr int SW = 64, LW = SW + 2;
constexpr int RPI = 2;                    // dY rows per interval
constexpr int NRX = 8, NRD = 2 * RPI;     // ring rows: x rows m .. m + 3 are read while m + 4, m + 5 are staged
constexpr int XROW = LW * 16, DROW = SW * 128;
constexpr int XRING = NRX * XROW, DRING = NRD * DROW;
constexpr int SLAB = 9 * 8 * 64;          // floats per workgroup partial
__device__ __forceinline__ int slot_off(int col, int c8) { return col * 128 + ((((c8 >> 2) ^ (col >> 1)) & 1) << 6) + ((c8 & 3) << 4); }
}  // namespace wt

typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ s16x4 tr_read(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p));
}

struct WgThinArgs {
    const __bf16* x;        // (B, H, W, in_cs) bf16, the octet at channels c0 .. c0 + 7
    const __bf16* dout;     // (B, H, W, 64) bf16
    float* partial;         // [workgroups][9][8][64]
    int H, W, in_cs, c0, nseg, nstrips, nitems;
};

__global__ void __launch_bounds__(256) conv3x3_wgrad_thin_bf16_kernel(WgThinArgs a) {
    using namespace wt;
    __shared__ __attribute__((aligned(16))) char smem[XRING + DRING];
    char* xring = smem;
    char* dring = smem + XRING;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cot = wv & 1, kh = wv >> 1;
    const int h = lane >> 5, r = lane & 31;
    const int tq = (lane & 15) >> 2, tp = lane & 3, tg = (lane >> 4) & 1;
    const int H = a.H, W = a.W, xpb = a.in_cs * 2;

    // A operands: row 16 tg + 4 tp + e of tile t = (tap 4 t + 2 tg + (tp >> 1), channel 4 (tp & 1) + e); the lane's pixel is
    // 32 kh + 16 s + 8 h + tq (+ 4 for the second read), shifted by the tap's kx; the tap's ky picks the x row
    int ky[3], xo[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        int tap = 4 * t + 2 * tg + (tp >> 1);
        tap = tap > 8 ? 8 : tap;                // (tap slots 9..11: rows nobody stores)
        ky[t] = tap / 3;
        xo[t] = (32 * kh + 8 * h + tq + (tap - 3 * ky[t])) * 16 + (tp & 1) * 8;
    }
    const int doff = (32 * kh + 8 * h + tq) * 128 + (((cot ^ (tq >> 1)) & 1) << 6) + (tg * 16 + tp * 4) * 2;
    f32x16 acc[3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    // loader constants: dY slot tid + 256 j of an interval's 2 x 512; x slot tid of its 2 x 66
    const int c8 = tid & 7;
    int gd[4], ld[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int px = (tid + j * 256) >> 3, row = px >> 6, col = px & 63;
        gd[j] = (row * W + col) * 128 + 16 * c8;
        ld[j] = row * DROW + slot_off(col, c8);
    }
    const bool xlive = tid < 2 * LW;
    const int xr = tid >= LW ? 1 : 0, xc = tid - xr * LW;

    for (int item = blockIdx.x; item < a.nitems; item += gridDim.x) {
        const int seg = item % a.nseg, rest = item / a.nseg;
        const int strip = rest % a.nstrips, b = rest / a.nstrips;
        const int rows_lo = H / a.nseg, rows_rem = H % a.nseg;
        const int y0 = seg * rows_lo + (seg < rows_rem ? seg : rows_rem);
        const int R = rows_lo + (seg < rows_rem ? 1 : 0);          // >= 1 (host: nseg <= H)
        const int x0 = strip * SW;
        const int K = (R + RPI - 1) / RPI;
        const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<__bf16*>(a.x + (int64_t)b * H * W * a.in_cs + a.c0), 0, (int)(((int64_t)H * W * a.in_cs - a.c0) * 2), 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<__bf16*>(a.dout + (int64_t)b * H * W * 64), 0, (int)((int64_t)H * W * 128), 0x00020000);
        // x row m of the segment is image row y0 - 1 + m (m <= R + 1), LDS column c image column x0 - 1 + c; outside the image: zeros
        auto loadx = [&](int m0) __attribute__((always_inline)) {
            const int m = m0 + xr, gy = y0 - 1 + m, gx = x0 - 1 + xc;
            const bool ok = xlive & (m <= R + 1) & ((unsigned)gy < (unsigned)H) & ((unsigned)gx < (unsigned)W);
            return __builtin_amdgcn_raw_buffer_load_b128(rs_x, ok ? (gy * W + gx) * xpb : OOB, 0, 0);
        };
        auto storex = [&](u32x4 v, int m0) __attribute__((always_inline)) {
            if (xlive) *reinterpret_cast<u32x4*>(xring + ((m0 + xr) & (NRX - 1)) * XROW + xc * 16) = v;
        };
        auto loadd = [&](u32x4 (&d)[4], int k) __attribute__((always_inline)) {
            int ndr = R - RPI * k;
            ndr = ndr > RPI ? RPI : (ndr < 0 ? 0 : ndr);
            const int sd = ((y0 + RPI * k) * W + x0) * 128;
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_d, (tid + j * 256 < ndr * 512) ? gd[j] : OOB, ndr ? sd : 0, 0);
        };
        auto stored = [&](const u32x4 (&d)[4], int k) __attribute__((always_inline)) {
            int ndr = R - RPI * k;
            ndr = ndr > RPI ? RPI : (ndr < 0 ? 0 : ndr);
            char* dst = dring + ((RPI * k) & (NRD - 1)) * DROW;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (tid + j * 256 < ndr * 512) *reinterpret_cast<u32x4*>(dst + ld[j]) = d[j];
        };
        u32x4 xa, da[4];
        __syncthreads();                 // (the previous item's last interval has been read)
        xa = loadx(0);
        storex(xa, 0);
        xa = loadx(2);
        loadd(da, 0);
        storex(xa, 2);
        stored(da, 0);
        xa = loadx(4);
        loadd(da, 1);
        __syncthreads();
        for (int k = 0; k < K; ++k) {
            // dY rows n = 2k, 2k + 1 against x rows n .. n + 2
#pragma unroll
            for (int rr = 0; rr < RPI; ++rr) {
                const int n = RPI * k + rr;
                if (n < R) {
                    const char* dr = dring + (n & (NRD - 1)) * DROW + doff;
                    int xb[3];
#pragma unroll
                    for (int t = 0; t < 3; ++t) xb[t] = ((n + ky[t]) & (NRX - 1)) * XROW + xo[t];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        union { s16x4 q[2]; bf16x8 v; } ub;
                        ub.q[0] = tr_read(dr + s * 2048);
                        ub.q[1] = tr_read(dr + s * 2048 + 512);
#pragma unroll
                        for (int t = 0; t < 3; ++t) {
                            union { s16x4 q[2]; bf16x8 v; } ua;
                            ua.q[0] = tr_read(xring + xb[t] + s * 256);
                            ua.q[1] = tr_read(xring + xb[t] + s * 256 + 64);
                            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ua.v, ub.v, acc[t], 0, 0, 0);
                        }
                    }
                }
            }
            storex(xa, 2 * k + 4);
            stored(da, k + 1);
            xa = loadx(2 * k + 6);
            loadd(da, k + 2);
            __syncthreads();
        }
    }
    // C[row][co]: lane = co (r), register i -> row (i & 3) + 8 (i >> 2) + 4 h of the tile = (tap 4 t + (i >> 2), channel (i & 3) + 4 h).
    // Pixel half 1 hands its sums to pixel half 0 through LDS: one partial per workgroup, one order.
    float* red = reinterpret_cast<float*>(dring);
    __syncthreads();
    if (kh == 1) {
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) red[((cot * 48 + t * 16 + i) << 6) + lane] = acc[t][i];
    }
    __syncthreads();
    if (kh == 0) {
        float* pbase = a.partial + (int64_t)blockIdx.x * SLAB;
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int tap = 4 * t + (i >> 2), c = (i & 3) + 4 * h;
                if (tap < 9) pbase[(tap * 8 + c) * 64 + cot * 32 + r] = acc[t][i] + red[((cot * 48 + t * 16 + i) << 6) + lane];
            }
    }
}

}  // namespace

// the thin chunk of a bf16 3x3 weight gradient to 64 output channels goes to the kernel above: 65..72 real input channels on 96-channel
// pixels, strips of 64 columns, no input transform
bool conv_wgrad_thin_ok(int storage, int in_cs, int ci_real, int dout_cs, int ks, int B, int H, int W) {
    const char* e = diag_env("P4C_WGRAD_THIN");             // (A/B switch of the diagnostic build: 0 = the row-streaming kernel's thin chunk)
    if (e && e[0] == '0') return false;
    const char* r = diag_env("P4C_NO_WGRAD_ROWS");
    if (r && r[0] == '1') return false;
    return storage == P4C_BF16 && in_cs == 96 && ci_real > 64 && ci_real <= 72 && dout_cs == 64 && ks == 3 && W % wt::SW == 0 && B > 0 &&
           H > 0 && (int64_t)H * W * in_cs * 2 < (int64_t)1 << 31;
}

// workgroups (= partial slabs) of the thin job: two per CU the weight gradients run on, G being their workgroup count (make_layout:
// half of the CUs) -- 256 slabs of 18 KB at the benchmark shape against 128 x 147 KB of a full chunk
int conv_wgrad_thin_slots(int G, int B, int H, int W, int* nseg_out) {
    const int nstrips = W / wt::SW;
    int g = 2 * G;
    if (const char* e = diag_env("P4C_WGRAD_THIN_G")) { const int v = atoi(e); if (v > 0) g = v; }   // (tests: workgroup counts)
    if (g > 12 * G) g = 12 * G;          // the slabs lie behind the full chunk's G slots of [9][96][64] in the same region
    int nseg = g / (B * nstrips);
    nseg = nseg > H ? H : (nseg < 1 ? 1 : nseg);
    const int nitems = B * nstrips * nseg;
    if (nseg_out) *nseg_out = nseg;
    return g < nitems ? g : nitems;
}

int launch_conv3x3_wgrad_thin_bf16(const void* x, int in_cs, const void* dout, float* partial, int G, int B, int H, int W, hipStream_t stream,
                                   int* nslots_out) {
    int nseg = 1;
    const int nwg = conv_wgrad_thin_slots(G, B, H, W, &nseg);
    const int nstrips = W / wt::SW;
    const WgThinArgs a{(const __bf16*)x, (const __bf16*)dout, partial, H, W, in_cs, 64, nseg, nstrips, B * nstrips * nseg};
    hipLaunchKernelGGL(conv3x3_wgrad_thin_bf16_kernel, dim3(nwg), dim3(256), 0, stream, a);
    P4C_CHECK_LAUNCH("conv3x3_wgrad_thin_bf16");
    *nslots_out = nwg;
    return P4C_OK;
}

}  // namespace p4c

// single-op entry point (tests): y (B,H,W,64) bf16 in place += conv3x3 of the channels 64 .. cin-1 of x (B,H,W,x_cs) bf16 with the fp32
// master weight w [64][cin][3][3]; stat_partial: p4c_first_conv_tail_slots(B,H,W) slots of [2][64] per sample, or NULL
extern "C" int p4c_first_conv_tail_slots(int B, int H, int W) { return p4c::first_conv_tail_slots(B, H, W); }
extern "C" int p4c_first_conv_tail(const void* x, int x_cs, int cin, const float* w, void* y, float* stat_partial, int B, int H, int W,
                                   p4c_stream_t stream) {
    P4C_CHECK_ARG(x && w && y, "p4c_first_conv_tail: NULL pointer");
    P4C_CHECK_ARG(cin > 64 && cin <= 72 && x_cs >= 72 && x_cs % 8 == 0 && W % 32 == 0 && B > 0 && H > 0,
                  "p4c_first_conv_tail: 65..72 input channels on pixels of >= 72 channels (multiple of 8), W a multiple of 32");
    return p4c::launch_first_conv_tail(x, x_cs, cin, w, y, stat_partial, B, H, W, p4c::as_stream(stream));
}

// single-op entry points (tests, micro-benchmarks) of the whole first convolution: y (B,H,W,64) bf16 = conv3x3 of channels 0 .. cin-1 of
// x (B,H,W,x_cs) bf16 with the fp32 master weight w [64][cin][3][3], prepared here into a stream-ordered temporary.
//   p4c_first_conv_one: ONE launch of the row kernel (conv_rows.hip: THIN), y rounded once; stat_partial (or NULL):
//                       p4c_first_conv_one_slots(B,H,W) slots of [2][64] per sample
//   p4c_first_conv_two: row launch on channels 0..63 + tail, what P4C_FIRST_CONV_ONE=0 runs; slots: p4c_first_conv_tail_slots
namespace p4c {
namespace {
int first_conv_single_op(bool one, const void* x, int x_cs, int cin, const float* w, void* y, float* stat_partial, int B, int H, int W,
                         hipStream_t st) {
    void* img = nullptr;
    P4C_CHECK_HIP(hipMallocAsync(&img, first_conv_one_image_bytes(), st));
    PrepBatch pb;
    pb.n = 0;
    pb.bf16 = 1;
    pb.zero_words = nullptr;
    pb.n_zero = 0;
    pb.job[pb.n++] = {w, img, 64, cin, 9, 0, 64, 64};
    if (one) pb.job[pb.n++] = {w, (char*)img + 9 * 64 * 64 * 2, 64, cin, 6, 0, 64, 16, 1};
    int rc = prep_weights_batch(pb, st);
    if (rc == P4C_OK) {
        if (one) {
            rc = launch_first_conv_one(x, x_cs, img, y, stat_partial, B, H, W, st);
        } else {
            rc = launch_conv_bf16_rows_wide_pixels(x, x_cs, img, y, B, H, W, st);
            if (rc == P4C_OK) rc = launch_first_conv_tail(x, x_cs, cin, w, y, stat_partial, B, H, W, st);
        }
    }
    (void)hipFreeAsync(img, st);
    return rc;
}
}  // namespace
}  // namespace p4c
extern "C" long long p4c_first_conv_launch_count(void) { return p4c::first_conv_launches(); }
extern "C" int p4c_first_conv_one_slots(int B, int H, int W) { return p4c::conv_rows_stat_slots(B, H, W); }
extern "C" int p4c_first_conv_one(const void* x, int x_cs, int cin, const float* w, void* y, float* stat_partial, int B, int H, int W,
                                  p4c_stream_t stream) {
    P4C_CHECK_ARG(x && w && y, "p4c_first_conv_one: NULL pointer");
    P4C_CHECK_ARG(cin > 64 && cin <= 72 && x_cs >= 72 && x_cs % 8 == 0 && W % 32 == 0 && B > 0 && H > 0,
                  "p4c_first_conv_one: 65..72 input channels on pixels of >= 72 channels (multiple of 8), W a multiple of 32");
    return p4c::first_conv_single_op(true, x, x_cs, cin, w, y, stat_partial, B, H, W, p4c::as_stream(stream));
}
extern "C" int p4c_first_conv_two(const void* x, int x_cs, int cin, const float* w, void* y, float* stat_partial, int B, int H, int W,
                                  p4c_stream_t stream) {
    P4C_CHECK_ARG(x && w && y, "p4c_first_conv_two: NULL pointer");
    P4C_CHECK_ARG(cin > 64 && cin <= 72 && x_cs >= 72 && x_cs % 8 == 0 && W % 32 == 0 && B > 0 && H > 0,
                  "p4c_first_conv_two: 65..72 input channels on pixels of >= 72 channels (multiple of 8), W a multiple of 32");
    return p4c::first_conv_single_op(false, x, x_cs, cin, w, y, stat_partial, B, H, W, p4c::as_stream(stream));
}
