// GRIB2 simple packing (data representation template 5.0) of the forecast, on the device: what predict_step's save_gribs
// (py4cast/lightning.py:1183-1187, io/outputs.py:116-220) hands to its host library field by field -- un-normalise, one strided plane
// per (lead time, feature) pulled with a blocking copy, range and packing on the host -- as one range pass and one pack pass over the
// NORMALISED prediction.  The host keeps the few dozen header octets of a message (py4cast_amd/grib2.py).
//
//   p4c_grib_pack   reads the prediction (B,T,N,F) features-last (strides as p4c_forecast_frames takes them) of the n accepted
//                   samples and writes, for every packed feature k of K with spec[k] = (D, nbits),
//                       params (n,T,K,5) int32   {vmin, vmax, R as fp32 bits; E; bad}
//                       packed (n,T,K,pitch) bytes: the first ceil(N nbits / 8) of a row are the data section's bit stream.
//
// One field (s,t,k), feature f = features[k] -- the contract tests/grib2_reference.py restates:
//   v    = pred * std[f], rounded; + mean[f], rounded (the two steps of p4c_unnormalize_planes: built with -ffp-contract=off);
//   vmin, vmax  min / max of the finite v ((NaN, NaN) without one); bad = the number of v that are not finite.  What the stream of a
//        field with bad > 0 holds is unspecified;
//   s(v) = v * 10^D for D >= 0, v / 10^-D for D < 0, in float64 (10^|D| is exact for |D| <= 15);
//   R    = the largest binary32 <= s(vmin);
//   E    = the smallest integer with ldexp(s(vmax) - R, -E) <= 2^nbits - 1; 0 when vmax == vmin (or nothing is finite);
//   X    = min(floor(ldexp(s(v) - R, -E) + 0.5), 2^nbits - 1): every operation a single rounded one in float64;
//   stream = X of stream point 0, 1, ... in nbits bits each, most significant bit first, the last octet zero-padded.  Stream point
//        q = r W + x is grid point (r, x), or (H-1-r, x) with flip_rows.  A decoded value is (R + X 2^E) / 10^D.
//
// Three launches on one stream, no host round trip, no atomics (min / max are exact in any order, the bad counts are integer sums
// in a fixed order: two calls give the same bytes):
//   range   a workgroup walks tiles of ONE (sample, lead time) with a grid stride; per-wave LDS slots -> block partial in the
//           caller's workspace.  Tiles are GP_TILE consecutive GRID points (the order does not matter here).
//   finish  grid (K, n*T), one wave: partials -> params, R and E in float64.
//   pack    tiles are GP_TILE consecutive STREAM points; a lane owns 8 consecutive stream points of one field -- nbits whole
//           octets -- assembles them in registers and stores them: 32-bit words where nbits is a multiple of 4 (8, 12, 16, 24, 32
//           reduce to shifts and byte permutes with compile-time positions), bytes for the other widths and for the ragged last
//           group of a field whose N is no multiple of 8.
// Two forms of the read side, as in forecast_frames.hip (grib_dense): dense -- the (points x F) block of a tile is read once in
// 16-byte loads and transposed through LDS (with flip_rows a stream tile is one contiguous segment per grid row it touches);
// gather -- only the K packed features are read.  In LDS point p sits in row (p & 7) * 16 + (p >> 3) of an odd pitch: the lanes of
// a field's 16 octet groups read consecutive rows.
#include "grib_pack_common.hpp"

using namespace p4c;

extern "C" int p4c_grib_tile(void) { return GP_TILE; }
extern "C" int p4c_grib_max_blocks(void) { return GP_MAX_BLOCKS; }
extern "C" int p4c_grib_max_features(void) { return GP_MAX_FEATURES; }
extern "C" int p4c_grib_max_samples(void) { return GP_MAX_SAMPLES; }
extern "C" int p4c_grib_pack_dense(int K, int F) { return grib_dense(K, F) ? 1 : 0; }

extern "C" size_t p4c_grib_pack_workspace_bytes(int n, int T, int64_t N, int K) {
    if (n < 1 || T < 1 || N < 1 || K < 1) return 0;
    return (size_t)n * (size_t)T * (size_t)grib_blocks_per_field_set(n, T, N) * (size_t)K * 3 * sizeof(float);
}

extern "C" int p4c_grib_pack(const float* pred, int64_t pred_bs, int64_t pred_ts, const int32_t* samples, const float* std,
                             const float* mean, const int32_t* features, const int32_t* spec, int flip_rows, int32_t* params,
                             unsigned char* packed, int64_t pitch, void* workspace, int B, int n, int T, int H, int W, int F, int K,
                             p4c_stream_t stream) {
    P4C_CHECK_ARG(pred && samples && std && mean && features && spec && params && packed && workspace, "p4c_grib_pack: null pointer");
    P4C_CHECK_ARG(B > 0 && n > 0 && n <= GP_MAX_SAMPLES && T > 0 && H > 0 && W > 0 && F > 0 && (int64_t)n * T <= 65535,
                  "p4c_grib_pack: bad dims (B=%d n=%d T=%d H=%d W=%d F=%d; n <= %d, n*T <= 65535)", B, n, T, H, W, F, GP_MAX_SAMPLES);
    P4C_CHECK_ARG(K > 0 && K <= GP_MAX_FEATURES, "p4c_grib_pack: %d features: 1 .. at most %d per call", K, GP_MAX_FEATURES);
    P4C_CHECK_ARG((reinterpret_cast<uintptr_t>(packed) & 3) == 0 && pitch > 0 && (pitch & 3) == 0,
                  "p4c_grib_pack: packed must be 4-byte aligned and its pitch (%lld) a positive multiple of 4", (long long)pitch);
    const int64_t N = (int64_t)H * W;
    P4C_CHECK_ARG(N < ((int64_t)1 << 31), "p4c_grib_pack: %lld grid points: at most 2^31 - 1", (long long)N);
    GpSpec sp;
    int64_t longest = 0;
    for (int k = 0; k < K; ++k) {
        const int D = spec[2 * k], nbits = spec[2 * k + 1];
        P4C_CHECK_ARG(D >= -GP_MAX_D && D <= GP_MAX_D && nbits >= 1 && nbits <= 32,
                      "p4c_grib_pack: spec %d: D = %d, nbits = %d (|D| <= %d and 1 <= nbits <= 32)", k, D, nbits, GP_MAX_D);
        sp.d[k] = (int8_t)D;
        sp.nbits[k] = (uint8_t)nbits;
        const int64_t bytes = (N * nbits + 7) / 8;
        if (bytes > longest) longest = bytes;
    }
    for (int k = K; k < GP_MAX_FEATURES; ++k) {
        sp.d[k] = 0;
        sp.nbits[k] = 8;
    }
    P4C_CHECK_ARG(pitch >= longest, "p4c_grib_pack: a pitch of %lld bytes for a stream of %lld", (long long)pitch, (long long)longest);
    // n*T <= 65535 and K <= 256: the product stays far below 2^63
    P4C_CHECK_ARG(pitch < ((int64_t)1 << 31) && (int64_t)n * T * K * pitch < ((int64_t)1 << 31),
                  "p4c_grib_pack: %lld stream bytes: at most 2^31 - 1 per call", (long long)((int64_t)n * T * K * pitch));
    GpSamples smp;
    for (int i = 0; i < n; ++i) {
        P4C_CHECK_ARG(samples[i] >= 0 && samples[i] < B, "p4c_grib_pack: sample %d of a batch of %d", (int)samples[i], B);
        smp.b[i] = samples[i];
    }
    for (int i = n; i < GP_MAX_SAMPLES; ++i) smp.b[i] = 0;
    // the rule of forecast_frames.hip: whole points in 16-byte loads when at least half of at most 64 features are packed
    const bool dense = grib_dense(K, F);
    const int nb = grib_blocks_per_field_set(n, T, N);
    const dim3 grid((unsigned)nb, (unsigned)(n * T)), block(GP_THREADS);
    hipStream_t st = as_stream(stream);
    float* partial = (float*)workspace;
    if (dense)
        hipLaunchKernelGGL(grib_range_kernel<true>, grid, block, 0, st, pred, pred_bs, pred_ts, smp, std, mean, features, partial, T, N, F, K);
    else
        hipLaunchKernelGGL(grib_range_kernel<false>, grid, block, 0, st, pred, pred_bs, pred_ts, smp, std, mean, features, partial, T, N, F, K);
    P4C_CHECK_LAUNCH("p4c_grib_pack(range)");
    hipLaunchKernelGGL(grib_finish_kernel<GP_PARAMS>, dim3((unsigned)K, (unsigned)(n * T)), dim3(64), 0, st, (const float*)partial, sp, params, nb, K);
    P4C_CHECK_LAUNCH("p4c_grib_pack(finish)");
    if (dense)
        hipLaunchKernelGGL(grib_pack_kernel<true>, grid, block, 0, st, pred, pred_bs, pred_ts, smp, std, mean, features, sp,
                           (const int32_t*)params, packed, pitch, flip_rows ? 1 : 0, T, (int)N, F, K, H, W);
    else
        hipLaunchKernelGGL(grib_pack_kernel<false>, grid, block, 0, st, pred, pred_bs, pred_ts, smp, std, mean, features, sp,
                           (const int32_t*)params, packed, pitch, flip_rows ? 1 : 0, T, (int)N, F, K, H, W);
    P4C_CHECK_LAUNCH("p4c_grib_pack(pack)");
    return P4C_OK;
}
