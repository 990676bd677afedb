// Native-grid planes onto the training sub-domain on the device: Titan's fit_to_grid (datasets/titan/__init__.py:184-208:
// crop to the AROME box, skimage.transform.resize to the target grid's full size), the latitude flip of load_data_for_date
// and the sub-domain cut of titan_cli.py, fused with the standardisation and the features-last pack of
// p4c_pack_standardize.  Only the sub-domain's pixels are computed; no full-grid plane exists.
//
// The definition is the scipy.ndimage form of resize: an optional separable Gaussian with mirror edges, then
// an order-1 zoom with grid_mode=True and mirror edges.  Everything that depends on the geometry alone is a host table
// (py4cast_amd/regrid.py, exact integer coordinates rounded to fp32 once):
//   * per output row and per output column of the sub-domain one tap entry (i0, i1, f), the flip and the sub-domain
//     origin folded in, the mirror already applied;
//   * for the blur the mirrored source index of every position -r .. n-1+r and the normalised weights.
// So regrid_pack_kernel holds no coordinate arithmetic: two table look-ups, four loads, three fused multiply-adds.  Its only
// divisions are the split of the block's first row into (b, t, y, x), once per block, and the IEEE d / std of the
// standardisation (this file is built with -ffp-contract=off: the two rounded steps of pack_standardize_kernel; the blend's
// fmaf calls are explicit).
//
// Layout as pack_standardize_kernel (rollout.hip): a block transposes 256 rows x F columns through LDS, so its output is one
// contiguous, ordered run of 256*F floats.  A row is ((b*T + t)*H + y)*W + x and a block may straddle (b, t) planes.
#include "common.hpp"

namespace p4c {

constexpr int RG_ROWS = 256;
constexpr int RG_MAX_COLS = 144;
constexpr int RG_TRIP = 4;          // features per trip: 16 independent loads of a thread in flight together
constexpr int RG_MAX_RADIUS = 64;
constexpr int BLUR_TH = 16, BLUR_TW = 64;

typedef __attribute__((address_space(1))) float gfloat;

__device__ __forceinline__ float lerp1(float a, float b, float f) { return fmaf(f, b - a, a); }

__global__ void __launch_bounds__(256)
    regrid_pack_kernel(const p4c_regrid_feature* __restrict__ feats, const p4c_regrid_tap* __restrict__ taps, float* __restrict__ out,
                       int64_t R, int T, int H, int W, int F) {
    extern __shared__ float tile[];  // [F][RG_ROWS + 1]: the + 1 keeps the transposed reads off one bank
    const int64_t r0 = (int64_t)blockIdx.x * RG_ROWS;
    const int64_t r = r0 + threadIdx.x;
    // (b, t, y, x) of the block's first row once per block (uniform; R < 2^31 is checked by the host), then a walk from there
    const uint32_t HW = (uint32_t)H * (uint32_t)W;
    const uint32_t bt0 = (uint32_t)r0 / HW, p0 = (uint32_t)r0 - bt0 * HW;
    const uint32_t y0 = p0 / (uint32_t)W;
    int b = (int)(bt0 / (uint32_t)T);
    int t = (int)bt0 - b * T, y = (int)y0, x = (int)(p0 - y0 * (uint32_t)W) + (int)threadIdx.x;
    while (x >= W) { x -= W; ++y; }
    while (y >= H) {
        y -= H;
        if (++t == T) { t = 0; ++b; }
    }
    if (r >= R) b = t = y = x = 0;   // rows past the end read plane 0's first pixel and store nothing
    // Features come sorted by tap table (any order is correct, this one reads each table once): the two entries of a row are
    // loaded once per run of features on one table.  The planes are device memory: loads through the global address space.
    const int per_table = H + W;
    int f0 = 0;
    while (f0 < F) {
        const int table = feats[f0].table;
        int f1 = f0 + 1;
        while (f1 < F && feats[f1].table == table) ++f1;
        const p4c_regrid_tap* tab = taps + (int64_t)table * per_table;
        const p4c_regrid_tap rt = tab[y], ct = tab[H + x];
        for (; f0 < f1; f0 += RG_TRIP) {
            float v[RG_TRIP][4];
#pragma unroll
            for (int k = 0; k < RG_TRIP; ++k) {
                const p4c_regrid_feature& d = feats[f0 + k < f1 ? f0 + k : f1 - 1];
                const gfloat* p = (const gfloat*)d.src + (int64_t)b * d.b_stride + (int64_t)t * d.t_stride + d.col0;
                const gfloat* top = p + (int64_t)(d.row0 + rt.i0) * d.pitch;
                const gfloat* bot = p + (int64_t)(d.row0 + rt.i1) * d.pitch;
                v[k][0] = top[ct.i0];
                v[k][1] = top[ct.i1];
                v[k][2] = bot[ct.i0];
                v[k][3] = bot[ct.i1];
            }
#pragma unroll
            for (int k = 0; k < RG_TRIP; ++k)
                if (f0 + k < f1) {
                    const p4c_regrid_feature& d = feats[f0 + k];
                    const float val = lerp1(lerp1(v[k][0], v[k][1], ct.f), lerp1(v[k][2], v[k][3], ct.f), rt.f);
                    const float c = val - d.mean;
                    tile[d.channel * (RG_ROWS + 1) + threadIdx.x] = c / d.std;      // rows past the end: computed, never stored
                }
        }
        f0 = f1;
    }
    __syncthreads();
    const int64_t rows_here = (R - r0 < RG_ROWS) ? (R - r0) : RG_ROWS;
    const int64_t total = rows_here * F;
    float* dst = out + r0 * F;
    int row = threadIdx.x / F, f = threadIdx.x - row * F;
    const int drow = 256 / F, df = 256 - drow * F;
    for (int64_t j = threadIdx.x; j < total; j += 256) {
        dst[j] = tile[f * (RG_ROWS + 1) + row];
        row += drow;
        f += df;
        if (f >= F) { f -= F; ++row; }
    }
}

// Separable Gaussian over one windowed plane, axis 0 then axis 1 as scipy.ndimage.gaussian_filter runs them.  A block makes a
// 16 x 64 output tile.  It stages the tile with its halo, (16 + 2 ry) x (64 + 2 rx) source pixels through the mirrored index
// tables, in LDS (a wave reads consecutive columns of one source row), runs the axis-0 pass LDS to LDS for the 64 + 2 rx
// columns, then the axis-1 pass to global memory; lanes walk consecutive columns in all three, so no LDS access conflicts.
// Sums run in tap order -r .. r, one fma per tap.
__global__ void __launch_bounds__(256)
    regrid_blur_kernel(const float* __restrict__ src, int64_t plane_stride, int pitch, int row0, int col0, float* __restrict__ dst,
                       int n, int m, const int* __restrict__ row_index, const int* __restrict__ col_index,
                       const float* __restrict__ row_w, int ry, const float* __restrict__ col_w, int rx) {
    extern __shared__ float lds[];     // halo [BLUR_TH + 2 ry][wide], then mid [BLUR_TH][wide]
    const int wide = BLUR_TW + 2 * rx, tall = BLUR_TH + 2 * ry;
    float* halo = lds;
    float* mid = lds + tall * wide;
    const gfloat* plane = (const gfloat*)src + (int64_t)blockIdx.z * plane_stride + (int64_t)row0 * pitch + col0;
    float* outp = dst + (int64_t)blockIdx.z * n * m;
    const int ty0 = blockIdx.y * BLUR_TH, tx0 = blockIdx.x * BLUR_TW;
    const int tx = threadIdx.x & 63, tq = threadIdx.x >> 6;      // a wave per row, four rows at a time
    for (int yy = tq; yy < tall; yy += 4) {
        const int ypos = ty0 + yy;                                  // indexes row_index: position ty0 + yy - ry of the plane
        const bool row_ok = ypos < n + 2 * ry;
        const int64_t roff = row_ok ? (int64_t)row_index[ypos] * pitch : 0;
        for (int j = tx; j < wide; j += 64) {
            const int xpos = tx0 + j;                               // indexes col_index likewise
            halo[yy * wide + j] = (row_ok && xpos < m + 2 * rx) ? plane[roff + col_index[xpos]] : 0.f;
        }
    }
    __syncthreads();
    for (int yy = tq; yy < BLUR_TH; yy += 4)
        for (int j = tx; j < wide; j += 64) {
            float acc = 0.f;
            for (int k = 0; k <= 2 * ry; ++k) acc = fmaf(row_w[k], halo[(yy + k) * wide + j], acc);
            mid[yy * wide + j] = acc;
        }
    __syncthreads();
    const int xo = tx0 + tx;
    for (int yy = tq; yy < BLUR_TH; yy += 4) {
        const int y = ty0 + yy;
        if (y < n && xo < m) {
            float acc = 0.f;
            for (int k = 0; k <= 2 * rx; ++k) acc = fmaf(col_w[k], mid[yy * wide + tx + k], acc);
            outp[(int64_t)y * m + xo] = acc;
        }
    }
}

}  // namespace p4c

using namespace p4c;

extern "C" int p4c_regrid_pack(const p4c_regrid_feature* feats, const p4c_regrid_tap* taps, float* out, int B, int T, int H_sub,
                               int W_sub, int F, p4c_stream_t stream) {
    static_assert(sizeof(p4c_regrid_feature) == 56 && sizeof(p4c_regrid_tap) == 16, "descriptor layout is part of the ABI");
    P4C_CHECK_ARG(F >= 1 && F <= RG_MAX_COLS, "p4c_regrid_pack: %d features: at most %d per call (LDS tile)", F, RG_MAX_COLS);
    P4C_CHECK_ARG(feats && taps && out, "p4c_regrid_pack: null pointer");
    P4C_CHECK_ARG(B > 0 && T > 0 && H_sub > 0 && W_sub > 0, "p4c_regrid_pack: bad dims (B=%d T=%d H=%d W=%d)", B, T, H_sub, W_sub);
    const int64_t rows = (int64_t)B * T * H_sub * W_sub;
    P4C_CHECK_ARG(rows < ((int64_t)1 << 31), "p4c_regrid_pack: %lld rows: at most 2^31 - 1 per call", (long long)rows);
    const size_t smem = (size_t)F * (RG_ROWS + 1) * sizeof(float);
    P4C_TRY(ensure_dyn_smem((const void*)regrid_pack_kernel, RG_MAX_COLS * (RG_ROWS + 1) * 4));
    hipLaunchKernelGGL(regrid_pack_kernel, dim3((unsigned)((rows + RG_ROWS - 1) / RG_ROWS)), dim3(256), smem, as_stream(stream), feats,
                       taps, out, rows, T, H_sub, W_sub, F);
    P4C_CHECK_LAUNCH("p4c_regrid_pack");
    return P4C_OK;
}

extern "C" int p4c_regrid_blur(const float* src, int64_t plane_stride, int pitch, int row0, int col0, float* dst, int planes, int n,
                               int m, const int* row_index, const int* col_index, const float* row_w, int ry, const float* col_w,
                               int rx, p4c_stream_t stream) {
    P4C_CHECK_ARG(ry >= 0 && rx >= 0 && ry <= RG_MAX_RADIUS && rx <= RG_MAX_RADIUS,
                  "p4c_regrid_blur: radius %d x %d: at most %d per axis", ry, rx, RG_MAX_RADIUS);
    P4C_CHECK_ARG(n >= 2 && m >= 2, "p4c_regrid_blur: a %d x %d plane: each axis needs at least 2 points (mirror period 2(n - 1))", n, m);
    P4C_CHECK_ARG(src && dst && row_index && col_index && row_w && col_w, "p4c_regrid_blur: null pointer");
    P4C_CHECK_ARG(planes > 0 && planes <= 65535, "p4c_regrid_blur: %d planes: 1 .. 65535 per call", planes);
    P4C_CHECK_ARG(row0 >= 0 && col0 >= 0 && pitch >= col0 + m && plane_stride >= (int64_t)(row0 + n) * pitch,
                  "p4c_regrid_blur: window %d+%d x %d+%d does not fit pitch %d / plane stride %lld", row0, n, col0, m, pitch,
                  (long long)plane_stride);
    const dim3 grid((unsigned)((m + BLUR_TW - 1) / BLUR_TW), (unsigned)((n + BLUR_TH - 1) / BLUR_TH), (unsigned)planes);
    P4C_CHECK_ARG(grid.y <= 65535, "p4c_regrid_blur: %d rows: at most %d per plane", n, 65535 * BLUR_TH);
    const size_t smem = (size_t)(2 * BLUR_TH + 2 * ry) * (BLUR_TW + 2 * rx) * sizeof(float);
    P4C_TRY(ensure_dyn_smem((const void*)regrid_blur_kernel, (2 * BLUR_TH + 2 * RG_MAX_RADIUS) * (BLUR_TW + 2 * RG_MAX_RADIUS) * 4));
    hipLaunchKernelGGL(regrid_blur_kernel, grid, dim3(256), smem, as_stream(stream), src, plane_stride, pitch, row0, col0, dst, n, m,
                       row_index, col_index, row_w, ry, col_w, rx);
    P4C_CHECK_LAUNCH("p4c_regrid_blur");
    return P4C_OK;
}
