// The training sub-domain decoded straight out of GRIB2 simple packing (data representation template 5.0): for fields that are
// already on the target grid, p4c_grib_unpack (full fp32 native planes) followed by p4c_regrid_pack (an identity tap table: the
// latitude flip, the sub-domain, the standardisation and the features-last pack) in ONE launch.  Simple packing without a bitmap is
// random access -- value p lies at bit p * nbits --, so only the rows of the sub-domain are shipped (grib2.window_slice), only the
// window's values are decoded, and no native plane exists.
//
//   p4c_grib_window_pack   B*T*F fields (p4c_grib_wfield, include/py4cast_hip.h) -> out (B,T,H,W,F) fp32 features-last.
//
// One output element (b, t, y, x, f), field d = fields[(b*T + t)*F + f] -- the contract grib2.unpack_window restates in numpy:
//   p      = (row0 + y*row_step) * ni + col0 + x: the stream point (the caller folds the latitude flip, the scanning direction and
//            the sub-domain origin into row0 / row_step / col0);
//   X      the nbits-bit big-endian integer at bit p*nbits - bit0 of the shipped slice (0 for nbits == 0);
//   v      float( (R + ldexp(X, E)) / 10^D )  (D >= 0;  * 10^-D otherwise): float64, every operation a single rounded one, exactly
//          the value of grib_unpack.hip (10^|D| is exact for |D| <= 15);
//   out    c = v - mean; c / std: two rounded fp32 steps (built with -ffp-contract=off), as regrid_pack_kernel and
//          pack_standardize_kernel do.  With mean 0 and std 1 this is v unchanged.
// So the result has the bits of the two-launch route: its bilinear blend of an identity plan is fmaf(0, b - a, a) = a.
//
// Layout as regrid_pack_kernel: a workgroup takes 256 consecutive output rows r = ((b*T + t)*H + y)*W + x and F features through an
// LDS tile padded to rows + 1, and writes one contiguous, ordered run of 256*F floats.  Lanes walk consecutive x, so the bit
// positions of a wave are consecutive: its loads are one run of 64*nbits bits.  A workgroup whose rows lie in one (b, t) plane --
// all but every (H*W/256)-th -- reads its F descriptors through uniform addresses; one that straddles planes reads them per lane.
// 16 bits (what operational files mostly hold): one 2-byte load per value.  Any other width: a 64-bit window of two byte-swapped,
// 4-byte aligned words of the slice.  The eight-values-per-16-byte load of grib_unpack.hip's 16-bit path was not built and not
// measured: at an odd ni (AROME: 1121) every other row of a 16-bit stream is only 2-byte aligned, and what bounds this launch (its
// float64 arithmetic per value, the transposed LDS read-out or its 4*F bytes written per pixel) has not been measured either.
// No byte outside a field's slice is read: the host checks that every value of the window lies inside it, and the last, partial
// word of a slice is put together from its bytes.  No atomics: two calls give the same bits.
#include <math.h>

#include "common.hpp"

namespace p4c {

constexpr int GW_ROWS = 256;
constexpr int GW_MAX_COLS = 144;
constexpr int GW_MAX_D = 15;

__constant__ double gw_pow10[GW_MAX_D + 1] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};

// word i of a slice of `len` bytes as the big-endian number it is in the file; bytes past the end read as 0 and are not touched
__device__ __forceinline__ uint32_t gw_word(const unsigned char* __restrict__ s, int64_t i, int64_t len) {
    const int64_t at = 4 * i;
    if (at + 4 <= len) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(s + at));
    uint32_t w = 0u;
    for (int j = 0; j < 4; ++j)
        if (at + j < len) w |= (uint32_t)s[at + j] << (24 - 8 * j);
    return w;
}

// the standardised value of window pixel (y, x) of field d
__device__ __forceinline__ float gw_value(const unsigned char* __restrict__ bytes, const p4c_grib_wfield& d, int y, int x) {
    const int nbits = d.nbits;
    uint32_t X = 0u;
    if (nbits > 0) {
        const int64_t p = (int64_t)(d.row0 + y * d.row_step) * d.ni + d.col0 + x;
        const int64_t bit = p * nbits - d.bit0;             // inside the slice: checked by the host
        const unsigned char* __restrict__ s = bytes + d.slice_off;
        if (nbits == 16) {
            const uint32_t h = *reinterpret_cast<const uint16_t*>(s + (bit >> 3));   // slice_off and bit0 / 8 are multiples of 4
            X = ((h & 0xffu) << 8) | (h >> 8);
        } else {
            const int64_t at = bit >> 5;
            const int sh = (int)(bit & 31);
            const uint32_t hi = gw_word(s, at, d.slice_len);
            const uint32_t lo = sh + nbits > 32 ? gw_word(s, at + 1, d.slice_len) : 0u;
            const uint64_t window = ((uint64_t)hi << 32) | lo;
            X = (uint32_t)((window << sh) >> (64 - nbits));
        }
    }
    const double t = (double)d.R + ldexp((double)X, d.E);
    const double pw = gw_pow10[d.D >= 0 ? d.D : -d.D];
    const float v = (float)(d.D >= 0 ? t / pw : t * pw);
    const float c = v - d.mean;
    return c / d.std;
}

// the F features of pixel (y, x) of one (b, t) plane, whose descriptors start at `fp`, into column `col` of the tile
__device__ __forceinline__ void gw_pixel(const unsigned char* __restrict__ bytes, const p4c_grib_wfield* __restrict__ fp, int F, int y,
                                         int x, float* tile, int col) {
    for (int f = 0; f < F; ++f) tile[f * (GW_ROWS + 1) + col] = gw_value(bytes, fp[f], y, x);
}

__global__ void __launch_bounds__(256)
    grib_window_pack_kernel(const unsigned char* __restrict__ bytes, const p4c_grib_wfield* __restrict__ fields, float* __restrict__ out,
                            int64_t R, int H, int W, int F) {
    extern __shared__ float tile[];  // [F][GW_ROWS + 1]: the + 1 keeps the transposed reads off one bank
    const int64_t r0 = (int64_t)blockIdx.x * GW_ROWS;
    const int64_t r = r0 + threadIdx.x;
    const int64_t rows_here = (R - r0 < GW_ROWS) ? (R - r0) : GW_ROWS;
    // (bt, y, x) of the block's first row once per block (uniform; R < 2^31 is checked by the host), then a walk from there
    const uint32_t HW = (uint32_t)H * (uint32_t)W;
    const uint32_t bt0 = (uint32_t)r0 / HW, p0 = (uint32_t)r0 - bt0 * HW;
    const uint32_t bt1 = (uint32_t)(r0 + rows_here - 1) / HW;       // of the block's last row
    const uint32_t y0 = p0 / (uint32_t)W;
    int bt = (int)bt0, y = (int)y0, x = (int)(p0 - y0 * (uint32_t)W) + (int)threadIdx.x;
    while (x >= W) { x -= W; ++y; }
    while (y >= H) { y -= H; ++bt; }
    if (r >= R) { bt = (int)bt0; y = x = 0; }   // rows past the end decode the plane's first pixel and store nothing
    if (bt0 == bt1)
        gw_pixel(bytes, fields + (int64_t)bt0 * F, F, y, x, tile, threadIdx.x);       // uniform descriptor addresses
    else
        gw_pixel(bytes, fields + (int64_t)bt * F, F, y, x, tile, threadIdx.x);
    __syncthreads();
    const int64_t total = rows_here * F;
    float* dst = out + r0 * F;
    int row = threadIdx.x / F, f = threadIdx.x - row * F;
    const int drow = 256 / F, df = 256 - drow * F;
    for (int64_t j = threadIdx.x; j < total; j += 256) {
        dst[j] = tile[f * (GW_ROWS + 1) + row];
        row += drow;
        f += df;
        if (f >= F) { f -= F; ++row; }
    }
}

}  // namespace p4c

using namespace p4c;

extern "C" int p4c_grib_window_max_features(void) { return GW_MAX_COLS; }

extern "C" int p4c_grib_window_pack(const unsigned char* bytes, int64_t nbytes, const p4c_grib_wfield* fields,
                                    const p4c_grib_wfield* fields_host, float* out, int B, int T, int H, int W, int F, p4c_stream_t stream) {
    static_assert(sizeof(p4c_grib_wfield) == 72, "descriptor layout is part of the ABI");
    P4C_CHECK_ARG(F >= 1 && F <= GW_MAX_COLS, "p4c_grib_window_pack: %d features: at most %d per call (LDS tile)", F, GW_MAX_COLS);
    P4C_CHECK_ARG(bytes && fields && fields_host && out, "p4c_grib_window_pack: null pointer");
    P4C_CHECK_ARG((reinterpret_cast<uintptr_t>(bytes) & 3) == 0, "p4c_grib_window_pack: bytes must be 4-byte aligned");
    P4C_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && nbytes >= 0, "p4c_grib_window_pack: bad dims (B=%d T=%d H=%d W=%d, %lld bytes)", B, T,
                  H, W, (long long)nbytes);
    const int64_t rows = (int64_t)B * T * H * W;
    P4C_CHECK_ARG(rows < ((int64_t)1 << 31), "p4c_grib_window_pack: %lld rows: at most 2^31 - 1 per call", (long long)rows);
    const int64_t nfields = (int64_t)B * T * F;
    for (int64_t i = 0; i < nfields; ++i) {
        const p4c_grib_wfield& f = fields_host[i];
        const long long li = (long long)i;
        P4C_CHECK_ARG(f.bitmap_off == -1, "p4c_grib_window_pack: field %lld: bitmap_off = %lld: a field with a bitmap is no random access, "
                      "it goes through p4c_grib_unpack", li, (long long)f.bitmap_off);
        P4C_CHECK_ARG(f.nbits >= 0 && f.nbits <= 32 && f.D >= -GW_MAX_D && f.D <= GW_MAX_D,
                      "p4c_grib_window_pack: field %lld: nbits = %d, D = %d (0 <= nbits <= 32 and |D| <= %d)", li, f.nbits, f.D, GW_MAX_D);
        P4C_CHECK_ARG(f.slice_off >= 0 && (f.slice_off & 3) == 0 && f.bit0 >= 0 && (f.bit0 & 31) == 0,
                      "p4c_grib_window_pack: field %lld: slice_off = %lld, bit0 = %lld: not negative, multiples of 4 bytes", li,
                      (long long)f.slice_off, (long long)f.bit0);
        P4C_CHECK_ARG(f.slice_len >= 0 && f.slice_off <= nbytes && f.slice_len <= nbytes - f.slice_off,
                      "p4c_grib_window_pack: field %lld: the slice [%lld, +%lld) leaves the %lld bytes", li, (long long)f.slice_off,
                      (long long)f.slice_len, (long long)nbytes);
        P4C_CHECK_ARG(f.row_step == 1 || f.row_step == -1, "p4c_grib_window_pack: field %lld: row_step = %d (1 or -1)", li, f.row_step);
        const int64_t last = (int64_t)f.row0 + (int64_t)(H - 1) * f.row_step;
        const int64_t lo = last < f.row0 ? last : f.row0, hi = last < f.row0 ? f.row0 : last;
        P4C_CHECK_ARG(f.ni > 0 && f.col0 >= 0 && (int64_t)f.col0 + W <= f.ni && lo >= 0 && hi < ((int64_t)1 << 31),
                      "p4c_grib_window_pack: field %lld: window %d x %d at stream row %d (step %d), column %d of rows of %d points", li, H, W,
                      f.row0, f.row_step, f.col0, f.ni);
        // every bit of every value of the window lies inside the slice
        const int64_t first_bit = (lo * f.ni + f.col0) * f.nbits, end_bit = (hi * f.ni + f.col0 + W) * f.nbits;
        P4C_CHECK_ARG(f.nbits == 0 || (first_bit >= f.bit0 && end_bit - f.bit0 <= 8 * f.slice_len),
                      "p4c_grib_window_pack: field %lld: the window's bits [%lld, %lld) leave the slice of %lld bytes from bit %lld", li,
                      (long long)first_bit, (long long)end_bit, (long long)f.slice_len, (long long)f.bit0);
    }
    const size_t smem = (size_t)F * (GW_ROWS + 1) * sizeof(float);
    P4C_TRY(ensure_dyn_smem((const void*)grib_window_pack_kernel, GW_MAX_COLS * (GW_ROWS + 1) * 4));
    hipLaunchKernelGGL(grib_window_pack_kernel, dim3((unsigned)((rows + GW_ROWS - 1) / GW_ROWS)), dim3(256), smem, as_stream(stream), bytes,
                       fields, out, rows, H, W, F);
    P4C_CHECK_LAUNCH("p4c_grib_window_pack");
    return P4C_OK;
}
