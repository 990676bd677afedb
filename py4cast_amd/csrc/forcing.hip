// The forcing batch built on the device: Sample.load's `forcing` tensor (datasets/base.py:455-527) =
// the standardised external forcing parameters, then the five channels of generate_forcings (base.py:233-274 ->
// forcingutils.py): four date values per (sample, lead time) broadcast over the grid, and the top-of-atmosphere solar
// irradiance per pixel
//   cos_sza = sin(phi) sin(delta) + cos(phi) cos(delta) cos(omega),   omega = 15 deg * (utc_hour + lon/15 - 12)
//   toa     = max(0, 1366 * cos_sza)
// (Solar Engineering of Thermal Processes, eq. 1.6.1a / 1.6.2 / 1.6.3, as forcingutils.py:90-132 has them).
//
// Everything that depends on the date alone comes in a host table of 8 floats per (b, t): the four date values already
// rescaled to [0, 1], sin(delta), cos(delta), the UTC hour of day, one pad (py4cast_amd/forcings.py: time_table).
// Everything that depends on the grid alone comes in three planes: sin(phi), cos(phi), lon/15 (grid_tables).
//
// Layout as pack_standardize_kernel (rollout.hip): a block transposes 256 rows x (Fe + 5) columns through LDS, so the
// output is one contiguous, ordered run of 256*(Fe + 5) floats.  The Fe external columns are the same contiguous plane
// reads and the same expression (v - mean) / std (this file is built with -ffp-contract=off: bit-equal to
// p4c_pack_standardize); the five generated columns are filled per row.  A row is (b*T + t)*HW + pixel and a block may
// straddle a (b, t) boundary, so the table entry is looked up per row.
#include <math.h>

#include "common.hpp"

namespace p4c {

constexpr int FORC_ROWS = 256;
constexpr int FORC_GEN = 5;      // generated columns
constexpr int FORC_TABLE = 8;    // floats per (b, t) table entry
constexpr int FORC_MAX_COLS = 144;

__global__ void __launch_bounds__(256)
    build_forcing_kernel(const float* __restrict__ raw, int64_t plane_stride, const float* __restrict__ mean,
                         const float* __restrict__ std, const float* __restrict__ sin_lat, const float* __restrict__ cos_lat,
                         const float* __restrict__ lon_hours, const float* __restrict__ table, float* __restrict__ out,
                         int64_t R, int64_t HW, int Fe) {
    extern __shared__ float tile[];  // [Fe + 5][FORC_ROWS + 1]: the + 1 keeps the transposed reads off one bank
    const int F = Fe + FORC_GEN;
    const int64_t r0 = (int64_t)blockIdx.x * FORC_ROWS;
    const int64_t r = r0 + threadIdx.x;
    // 8 planes per trip: the 8 loads of a thread are independent and in flight together
    for (int f0 = 0; f0 < Fe; f0 += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (f0 + k < Fe && r < R) ? raw[(int64_t)(f0 + k) * plane_stride + r] : 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (f0 + k < Fe) {
                const float d = v[k] - mean[f0 + k];
                tile[(f0 + k) * (FORC_ROWS + 1) + threadIdx.x] = (r < R) ? d / std[f0 + k] : 0.f;
            }
    }
    if (r < R) {
        // (b, t) and pixel of the block's first row once per block (uniform: one division per wave, 32-bit where the rows
        // allow it), then a walk from there: a block crosses at most 256 / HW + 1 boundaries
        int64_t bt, pix;
        if (R <= 0x7fffffff) {
            const uint32_t q = (uint32_t)r0 / (uint32_t)HW;
            bt = q;
            pix = (int64_t)((uint32_t)r0 - q * (uint32_t)HW);
        } else {
            bt = r0 / HW;
            pix = r0 - bt * HW;
        }
        pix += threadIdx.x;
        while (pix >= HW) { pix -= HW; ++bt; }
        const float* e = table + bt * FORC_TABLE;
        float* col = tile + Fe * (FORC_ROWS + 1) + threadIdx.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) col[k * (FORC_ROWS + 1)] = e[k];
        // the hour angle leaves +-180 degrees (utc_hour + lon/15 - 12 spans -24 .. 36 h): the three-term sum is exact in
        // double, one step of 24 h brings it into +-12 h (cos has that period), and cosf sees an argument within +-pi
        double h = (double)e[6] + (double)lon_hours[pix] - 12.0;
        h = h > 12.0 ? h - 24.0 : (h < -12.0 ? h + 24.0 : h);
        const float omega = (float)(h * 0.26179938779914943654);  // 15 degrees per hour, in radians
        const float a = sin_lat[pix] * e[4];
        const float b = cos_lat[pix] * e[5];
        const float cos_sza = a + b * cosf(omega);
        col[4 * (FORC_ROWS + 1)] = fmaxf(0.f, 1366.f * cos_sza);
    }
    __syncthreads();
    const int64_t rows_here = (R - r0 < FORC_ROWS) ? (R - r0) : FORC_ROWS;
    const int64_t total = rows_here * F;
    float* dst = out + r0 * F;
    int row = threadIdx.x / F, f = threadIdx.x - row * F;
    const int drow = 256 / F, df = 256 - drow * F;
    for (int64_t j = threadIdx.x; j < total; j += 256) {
        dst[j] = tile[f * (FORC_ROWS + 1) + row];
        row += drow;
        f += df;
        if (f >= F) { f -= F; ++row; }
    }
}

}  // namespace p4c

using namespace p4c;

extern "C" int p4c_build_forcing(const float* raw, int64_t plane_stride, const float* mean, const float* std,
                                 const float* sin_lat, const float* cos_lat, const float* lon_hours, const float* time_table,
                                 float* out, int B, int T, int64_t HW, int Fe, p4c_stream_t stream) {
    P4C_CHECK_ARG(Fe >= 0 && Fe + FORC_GEN <= FORC_MAX_COLS,
                  "p4c_build_forcing: %d external + %d generated features: at most %d per call (LDS tile)", Fe, FORC_GEN, FORC_MAX_COLS);
    P4C_CHECK_ARG(sin_lat && cos_lat && lon_hours && time_table && out, "p4c_build_forcing: null pointer");
    P4C_CHECK_ARG(Fe == 0 || (raw && mean && std), "p4c_build_forcing: %d external features need raw, mean and std", Fe);
    P4C_CHECK_ARG(B > 0 && T > 0 && HW > 0 && HW <= (((int64_t)1 << 38) / B) / T, "p4c_build_forcing: bad dims (B=%d T=%d HW=%lld)", B, T,
                  (long long)HW);
    const int64_t rows = (int64_t)B * T * HW;
    P4C_CHECK_ARG(Fe == 0 || plane_stride >= rows, "p4c_build_forcing: plane stride %lld < %lld rows", (long long)plane_stride,
                  (long long)rows);
    const int F = Fe + FORC_GEN;
    const size_t smem = (size_t)F * (FORC_ROWS + 1) * sizeof(float);
    P4C_TRY(ensure_dyn_smem((const void*)build_forcing_kernel, FORC_MAX_COLS * (FORC_ROWS + 1) * 4));
    hipLaunchKernelGGL(build_forcing_kernel, dim3((unsigned)((rows + FORC_ROWS - 1) / FORC_ROWS)), dim3(256), smem, as_stream(stream),
                       raw, plane_stride, mean, std, sin_lat, cos_lat, lon_hours, time_table, out, rows, HW, Fe);
    P4C_CHECK_LAUNCH("p4c_build_forcing");
    return P4C_OK;
}
