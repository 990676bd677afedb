// GRIB2 complex packing (data representation template 5.2) and complex packing with spatial differencing (5.3) of the forecast, on
// the device: the opt-in route of the forecast writer beside p4c_grib_pack (grib_pack.hip), for templates whose messages are
// complex-packed.  The read forms, the quantisation and the range and finish passes are those of grib_pack.hip (grib_pack_common.hpp).
//
//   p4c_grib_pack_complex   reads the prediction as p4c_grib_pack does and writes, for every packed feature k of K with
//                           spec[k] = (D, nbits, order),
//                       params (n,T,K,11) int32  {vmin, vmax, R as fp32 bits; E; bad; ival1; ival2; gmin; ref_bits; length; offset}
//                       out    one byte buffer: the section-7 payload of field (s,t,k) is out[offset .. offset + length).
//
// One field of N stream points (flip_rows first), the contract py4cast_amd/grib2.py::pack_complex restates:
//   X      the integers of p4c_grib_pack, 0 <= X <= 2^nbits - 1;
//   d      order 0: d[q] = X[q];  1: d[q] = X[q] - X[q-1], q >= 1;  2: d[q] = X[q] - 2 X[q-1] + X[q-2], q >= 2;
//   gmin   min of d over q >= order (0 at order 0 and when there is no such q);  X'[q] = d[q] - gmin, 0 for q < order;
//   ival1 = X[0], ival2 = X[1] (order 2; 0 where the point does not exist or the order has none);
//   groups of 32 values, the last one N - 32 (ng - 1): ref[g] = min X', width[g] = the bits of max X' - min X';
//   ref_bits = the bits of the largest ref[g];
//   payload = descriptors (order >= 1: ival1, [ival2,] gmin, 4 octets each, sign and magnitude) | ng references of ref_bits bits |
//             ng widths of 6 bits | the values X' - ref[g] in width[g] bits, group after group; each part zero-padded to an octet.
//             A full group of width w is 4 w octets: every group starts on an octet.
//   length = the payload's octets, 0 for a field with bad > 0;  offset = the sum of the lengths, each rounded up to 4, of the fields
//            before it in (sample, lead time, feature) order.  Nothing is written outside the payloads.
// Limits: order 0 takes nbits 1 .. 32, orders 1 and 2 need nbits + order <= 31: every descriptor, X', reference fits 32 bits.
//
// Seven launches on one stream, no host round trip, no atomics, workgroups depend on each other through launch boundaries only:
//   range, finish   those of p4c_grib_pack -> the first five words of a params record;
//   group    tiles of GP_TILE stream points as in the pack pass of grib_pack.hip; a lane owns 8 consecutive points, quantises them and
//            the `order` points before them (from the tile, or from global memory across a tile or workgroup boundary), differences,
//            and four lanes fold min / max of d into the group's record in the workspace; the lane of point 0 writes ival1, ival2;
//   scan     one workgroup per field: gmin, then ref_bits and the first octet of every group's values (a block scan with a carry)
//            -> params words 5 .. 9;
//   offsets  one workgroup: the exclusive sum of the padded lengths -> params word 10;
//   tables   one workgroup per field: descriptors, references and widths, 8 groups -- whole octets -- per lane;
//   pack     a lane stores its 8 values of the group's width: w whole octets.  In the dense form the prediction is read and
//            quantised again, as in the group pass; in the gather form the group pass keeps its differences (4 bytes per value in
//            the workspace) and the pack pass reads those: the choice is measured (gc_stored below).
#include <limits.h>

#include "grib_pack_common.hpp"

namespace p4c {

constexpr int GC_GROUP = 32;             // values of a group
constexpr int GC_PARAMS = 11;            // int32 words of a params record
constexpr int GC_W_BITS = 6;             // bits of a stored group width
constexpr int GC_SCAN_THREADS = 256;
static_assert(GP_TILE % GC_GROUP == 0 && GC_GROUP == 4 * 8, "four lanes of 8 points make a group");

struct GcOrder {
    uint8_t o[GP_MAX_FEATURES];
};
struct GcGroup {   // min and max of d over the group's values q >= order; after the scan pass: of d with X' = 0 counted as gmin
    long long lo, hi;
};

__device__ __forceinline__ int gc_bits(unsigned long long v) { return v ? 64 - __clzll((long long)v) : 0; }

static inline int64_t gc_groups(int64_t N) { return (N + GC_GROUP - 1) / GC_GROUP; }
static inline int64_t gc_table_octets(int64_t ng, int bits) { return (ng * bits + 7) / 8; }
__device__ __forceinline__ int64_t gc_head(int order, int64_t ng, int ref_bits) {   // octets in front of the values
    return (order ? 4 * (order + 1) : 0) + ((ng * ref_bits + 7) >> 3) + ((ng * GC_W_BITS + 7) >> 3);
}

// the worst case of one field's payload, rounded up to 4
static inline int64_t gc_field_capacity(int64_t N, int nbits, int order) {
    const int64_t ng = gc_groups(N);
    const int64_t octets = (order ? 4 * (order + 1) : 0) + 4 * ng + gc_table_octets(ng, GC_W_BITS) + 4 * ng * (nbits + order);
    return (octets + 3) / 4 * 4;
}

// exclusive sum of v over the workgroup (GC_SCAN_THREADS threads) -> mine; total: the sum, in every thread
__device__ __forceinline__ uint32_t gc_block_scan(uint32_t v, uint32_t* wave_s, uint32_t& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();   // the previous scan's readers are done
    if (lane == 63) wave_s[wv] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < GC_SCAN_THREADS / 64; ++i) {
        if (i < wv) before += wave_s[i];
        total += wave_s[i];
    }
    return before + inc - v;
}

// grid (nb, n*T).  PACK = false: the group pass; true: the pack pass.  STORED (the A/B switch P4C_GRIB_CPX_STORED of the diag build):
// the group pass keeps the low 32 bits of every d (order 0: X itself; orders 1, 2: d fits an int32) in `dws`, field after field at a
// pitch of `dpitch` words, and the pack pass reads them instead of the prediction
template <bool DENSE, bool PACK, bool STORED>
__global__ void __launch_bounds__(GP_THREADS)
    grib_cpx_tile_kernel(const float* __restrict__ pred, int64_t pred_bs, int64_t pred_ts, const GpSamples smp,
                         const float* __restrict__ std, const float* __restrict__ mean, const int32_t* __restrict__ feats,
                         const GpSpec spec, const GcOrder ord, int32_t* __restrict__ params, GcGroup* __restrict__ groups,
                         const uint32_t* __restrict__ gstart, unsigned char* __restrict__ out, uint32_t* __restrict__ dws, int64_t dpitch,
                         int flip, int T, int N, int F, int K, int H, int W, int ng) {
    constexpr bool READS = !(PACK && STORED);   // this pass reads the prediction
    __shared__ float tile_s[DENSE && READS ? GP_TILE * (GP_DENSE_MAX_F + 1) : 1];
    const int tid = threadIdx.x;
    const int st = blockIdx.y, s = st / T, t = st - s * T;
    const float* base = pred + (int64_t)smp.b[s] * pred_bs + (int64_t)t * pred_ts;
    const int FP = F | 1;
    const int tiles = (N + GP_TILE - 1) / GP_TILE;
    const int units = K * GP_OCTS;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int q0 = tile * GP_TILE;
        const int pts = N - q0 < GP_TILE ? N - q0 : GP_TILE;
        if constexpr (DENSE && READS) {
            __syncthreads();
            if (!flip) {
                gp_load_segment(base + (int64_t)q0 * F, pts * F, F, FP, tile_s, tid, 0);
            } else {   // one contiguous piece per grid row the tile touches
                for (int p = 0; p < pts;) {
                    const int q = q0 + p, r = q / W, x = q - r * W;
                    const int len = W - x < pts - p ? W - x : pts - p;
                    gp_load_segment(base + ((int64_t)(H - 1 - r) * W + x) * F, len * F, F, FP, tile_s, tid, p);
                    p += len;
                }
            }
            __syncthreads();
        }
        // every thread takes every trip: the four lanes of a group meet in the shuffles below
        for (int u0 = 0; u0 < units; u0 += GP_THREADS) {
            const int u = u0 + tid;
            const int k = u / GP_OCTS, j = u - k * GP_OCTS, p0 = 8 * j;
            const bool live = u < units && p0 < pts;
            long long lo = LLONG_MAX, hi = LLONG_MIN;
            if (live) {
                const int f = feats[k];
                const float sd = std[f], mu = mean[f];
                const int D = spec.d[k], nbits = spec.nbits[k], order = ord.o[k];
                const int64_t field = (int64_t)st * K + k;
                int32_t* rec = params + field * GC_PARAMS;
                const double R = (double)__int_as_float(rec[2]);
                const int E = rec[3];
                const double pw = gp_pow10[D >= 0 ? D : -D];
                const double xmax = ldexp(1.0, nbits) - 1.0;
                const int valid = pts - p0 < 8 ? pts - p0 : 8;
                const int q = q0 + p0;
                long long d[8];
                [[maybe_unused]] long long x0 = 0, x1 = 0;   // X of stream points 0 and 1 (the lane of q = 0)
                if constexpr (READS) {
                    long long X[10];   // X[2 + i]: stream point q + i; X[1], X[0]: the two before q
                    X[0] = X[1] = 0;
    #pragma unroll
                    for (int h = 1; h <= 2; ++h) {
                        if (h <= order && q - h >= 0) {
                            float raw;
                            if (DENSE && p0 - h >= 0) {
                                raw = tile_s[gp_row(p0 - h) * FP + f];
                            } else {   // across a tile (or workgroup) boundary, and the gather form
                                const int qq = q - h, r = qq / W, x = qq - r * W;
                                raw = base[(flip ? (int64_t)(H - 1 - r) * W + x : (int64_t)qq) * F + f];
                            }
                            X[2 - h] = gp_quant(gp_value(raw, sd, mu), D, pw, R, E, xmax);
                        }
                    }
                    int r = 0, x = 0;
                    if constexpr (!DENSE) {
                        r = q / W;
                        x = q - r * W;
                    }
    #pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        X[2 + i] = 0;
                        if (i < valid) {
                            float raw;
                            if constexpr (DENSE) {
                                raw = tile_s[(i * GP_OCTS + j) * FP + f];
                            } else {
                                const int64_t g = flip ? (int64_t)(H - 1 - r) * W + x : (int64_t)q + i;
                                raw = base[g * F + f];
                                if (++x == W) {
                                    x = 0;
                                    ++r;
                                }
                            }
                            X[2 + i] = gp_quant(gp_value(raw, sd, mu), D, pw, R, E, xmax);
                        }
                    }
    #pragma unroll
                    for (int i = 0; i < 8; ++i)
                        d[i] = order == 0 ? X[2 + i] : order == 1 ? X[2 + i] - X[1 + i] : X[2 + i] - 2 * X[1 + i] + X[i];
                    x0 = X[2];
                    x1 = X[3];
                    if constexpr (STORED) {
                        uint32_t* dw = dws + field * dpitch + q;
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            if (i < valid) dw[i] = (uint32_t)d[i];
                    }
                } else {
                    const uint32_t* dw = dws + field * dpitch + q;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const uint32_t word = i < valid ? dw[i] : 0u;
                        d[i] = order == 0 ? (long long)word : (long long)(int32_t)word;
                    }
                }
                if constexpr (!PACK) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        if (i < valid && q + i >= order) {
                            lo = d[i] < lo ? d[i] : lo;
                            hi = d[i] > hi ? d[i] : hi;
                        }
                    }
                    if (q == 0 && order > 0) {
                        rec[5] = (int32_t)x0;
                        rec[6] = order == 2 && N > 1 ? (int32_t)x1 : 0;
                    }
                } else if (rec[4] == 0) {
                    const int g = (q0 / GC_GROUP) + (j >> 2);
                    const GcGroup gr = groups[field * ng + g];
                    const int w = gc_bits((unsigned long long)(gr.hi - gr.lo));
                    if (w > 0) {
                        uint32_t vals[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i) vals[i] = i < valid && q + i >= order ? (uint32_t)(d[i] - gr.lo) : 0u;
                        unsigned char* dst = out + rec[10] + gc_head(order, ng, rec[8]) + gstart[field * ng + g] + (j & 3) * w;
                        gp_store_bytes(dst, vals, w, valid == 8 ? w : (valid * w + 7) >> 3);
                    }
                }
            }
            if constexpr (!PACK) {
#pragma unroll
                for (int o = 1; o <= 2; o <<= 1) {
                    const long long l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
                    lo = l2 < lo ? l2 : lo;
                    hi = h2 > hi ? h2 : hi;
                }
                if (live && (j & 3) == 0) {
                    GcGroup gr;
                    gr.lo = lo;
                    gr.hi = hi;
                    groups[((int64_t)st * K + k) * ng + (q0 / GC_GROUP) + (j >> 2)] = gr;
                }
            }
        }
    }
}

// grid (fields): gmin, ref_bits, the first octet of every group's values, the field's length -> params words 5 .. 9
__global__ void __launch_bounds__(GC_SCAN_THREADS)
    grib_cpx_scan_kernel(const GcOrder ord, int32_t* __restrict__ params, GcGroup* __restrict__ groups, uint32_t* __restrict__ gstart,
                         int N, int K, int ng) {
    __shared__ long long red_s[GC_SCAN_THREADS / 64];
    __shared__ uint32_t wave_s[GC_SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t field = blockIdx.x;
    const int order = ord.o[field % K];
    int32_t* rec = params + field * GC_PARAMS;
    GcGroup* gr = groups + field * ng;
    uint32_t* gs = gstart + field * ng;
    long long m = LLONG_MAX;
    if (order)
        for (int g = tid; g < ng; g += GC_SCAN_THREADS) m = gr[g].lo < m ? gr[g].lo : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long m2 = __shfl_xor(m, o, 64);
        m = m2 < m ? m2 : m;
    }
    if (lane == 0) red_s[wv] = m;
    __syncthreads();
    m = red_s[0];
#pragma unroll
    for (int i = 1; i < GC_SCAN_THREADS / 64; ++i) m = red_s[i] < m ? red_s[i] : m;
    const long long gmin = m == LLONG_MAX ? 0 : m;   // order 0, or no value past the first `order`
    long long top = 0;
    uint32_t carry = 0;
    for (int g0 = 0; g0 < ng; g0 += GC_SCAN_THREADS) {
        const int g = g0 + tid;
        uint32_t octets = 0;
        if (g < ng) {
            GcGroup v = gr[g];
            if (order && g == 0) {   // the first `order` values are X' = 0: d = gmin
                v.lo = gmin;
                v.hi = v.hi > gmin ? v.hi : gmin;
                gr[0] = v;
            }
            const long long ref = v.lo - gmin;
            top = ref > top ? ref : top;
            const int w = gc_bits((unsigned long long)(v.hi - v.lo));
            const int len = g == ng - 1 ? N - GC_GROUP * (ng - 1) : GC_GROUP;
            octets = (uint32_t)((len * w + 7) >> 3);
        }
        uint32_t total;
        const uint32_t mine = gc_block_scan(octets, wave_s, total);
        if (g < ng) gs[g] = carry + mine;
        carry += total;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long t2 = __shfl_xor(top, o, 64);
        top = t2 > top ? t2 : top;
    }
    __syncthreads();   // red_s is read above
    if (lane == 0) red_s[wv] = top;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int i = 1; i < GC_SCAN_THREADS / 64; ++i) top = red_s[i] > top ? red_s[i] : top;
        const int ref_bits = gc_bits((unsigned long long)top);
        if (order == 0) rec[5] = 0;
        if (order != 2) rec[6] = 0;
        rec[7] = (int32_t)gmin;
        rec[8] = ref_bits;
        rec[9] = rec[4] ? 0 : (int32_t)(gc_head(order, ng, ref_bits) + carry);
    }
}

// one workgroup: the offset of every field, the padded lengths of the fields before it -> params word 10
__global__ void __launch_bounds__(GC_SCAN_THREADS) grib_cpx_offsets_kernel(int32_t* __restrict__ params, int64_t fields) {
    __shared__ uint32_t wave_s[GC_SCAN_THREADS / 64];
    uint32_t carry = 0;
    for (int64_t i0 = 0; i0 < fields; i0 += GC_SCAN_THREADS) {
        const int64_t i = i0 + threadIdx.x;
        const uint32_t len = i < fields ? ((uint32_t)params[i * GC_PARAMS + 9] + 3u) & ~3u : 0u;
        uint32_t total;
        const uint32_t mine = gc_block_scan(len, wave_s, total);
        if (i < fields) params[i * GC_PARAMS + 10] = (int32_t)(carry + mine);
        carry += total;
    }
}

__device__ __forceinline__ void gc_store_sm(unsigned char* dst, int v) {   // sign and magnitude, 4 octets, big-endian
    const uint32_t raw = v < 0 ? 0x80000000u | (uint32_t)(-(long long)v) : (uint32_t)v;
    dst[0] = (unsigned char)(raw >> 24);
    dst[1] = (unsigned char)(raw >> 16);
    dst[2] = (unsigned char)(raw >> 8);
    dst[3] = (unsigned char)raw;
}

// grid (fields): the descriptors and the two group tables of a payload; a lane takes 8 groups: ref_bits and 6 whole octets
__global__ void __launch_bounds__(GC_SCAN_THREADS)
    grib_cpx_tables_kernel(const GcOrder ord, const int32_t* __restrict__ params, const GcGroup* __restrict__ groups,
                           unsigned char* __restrict__ out, int K, int ng) {
    const int64_t field = blockIdx.x;
    const int order = ord.o[field % K];
    const int32_t* rec = params + field * GC_PARAMS;
    if (rec[4]) return;
    const GcGroup* gr = groups + field * ng;
    const long long gmin = rec[7];
    const int ref_bits = rec[8];
    unsigned char* dst = out + rec[10];
    if (threadIdx.x == 0 && order) {
        gc_store_sm(dst, rec[5]);
        if (order == 2) gc_store_sm(dst + 4, rec[6]);
        gc_store_sm(dst + 4 * order, rec[7]);
    }
    unsigned char* refs = dst + (order ? 4 * (order + 1) : 0);
    unsigned char* widths = refs + (((int64_t)ng * ref_bits + 7) >> 3);
    const int units = (ng + 7) >> 3;
    for (int u = threadIdx.x; u < units; u += GC_SCAN_THREADS) {
        const int g0 = 8 * u, cnt = ng - g0 < 8 ? ng - g0 : 8;
        uint32_t ref[8], wid[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            ref[i] = wid[i] = 0u;
            if (i < cnt) {
                const GcGroup v = gr[g0 + i];
                ref[i] = (uint32_t)(v.lo - gmin);
                wid[i] = (uint32_t)gc_bits((unsigned long long)(v.hi - v.lo));
            }
        }
        if (ref_bits) gp_store_bytes(refs + (int64_t)u * ref_bits, ref, ref_bits, cnt == 8 ? ref_bits : (cnt * ref_bits + 7) >> 3);
        gp_store_bytes(widths + (int64_t)u * GC_W_BITS, wid, GC_W_BITS, cnt == 8 ? GC_W_BITS : (cnt * GC_W_BITS + 7) >> 3);
    }
}

static inline size_t gc_align16(size_t b) { return (b + 15) / 16 * 16; }

// Whether the pack pass reads differences that the group pass stored, or the prediction again.  Measured
// (profiles/grib_pack_complex.txt): the gather form, which pays a 64-byte line per packed feature and point for every read of the
// prediction, is faster with stored differences (273 against 332 us at 2x3x512x640x21, 6 features); the dense form, which reads
// whole points once through LDS, is faster without the extra 4 bytes per value written and read (827 against 940 us at
// 2x3x512x512x60).
static inline bool gc_stored(bool dense) {
    const char* e = diag_env("P4C_GRIB_CPX_STORED");
    return e ? e[0] == '1' : !dense;
}
static inline size_t gc_dpitch(int64_t N) { return (size_t)(N + 7) / 8 * 8; }

}  // namespace p4c

using namespace p4c;

extern "C" int p4c_grib_pack_complex_group(void) { return GC_GROUP; }
extern "C" int p4c_grib_pack_complex_params(void) { return GC_PARAMS; }
extern "C" int p4c_grib_pack_complex_scan_threads(void) { return GC_SCAN_THREADS; }

extern "C" int64_t p4c_grib_pack_complex_capacity(int n, int T, int64_t N, const int32_t* spec, int K) {
    if (n < 1 || T < 1 || N < 1 || K < 1 || !spec) return -1;
    int64_t per_set = 0;
    for (int k = 0; k < K; ++k) {
        const int nbits = spec[3 * k + 1], order = spec[3 * k + 2];
        if (order < 0 || order > 2 || nbits < 1 || (order == 0 ? nbits > 32 : nbits + order > 31)) return -1;
        per_set += gc_field_capacity(N, nbits, order);
    }
    return (int64_t)n * T * per_set;
}

extern "C" size_t p4c_grib_pack_complex_workspace_bytes(int n, int T, int64_t N, int K, int F) {
    if (n < 1 || T < 1 || N < 1 || K < 1 || F < 1) return 0;
    const size_t fields = (size_t)n * (size_t)T * (size_t)K, ng = (size_t)gc_groups(N);
    const size_t partial = (size_t)n * (size_t)T * (size_t)grib_blocks_per_field_set(n, T, N) * (size_t)K * 3 * sizeof(float);
    return gc_align16(partial) + fields * ng * sizeof(GcGroup) + gc_align16(fields * ng * sizeof(uint32_t)) +
           (gc_stored(grib_dense(K, F)) ? fields * gc_dpitch(N) * sizeof(uint32_t) : 0);
}

extern "C" int p4c_grib_pack_complex(const float* pred, int64_t pred_bs, int64_t pred_ts, const int32_t* samples, const float* std,
                                     const float* mean, const int32_t* features, const int32_t* spec, int flip_rows, int32_t* params,
                                     unsigned char* out, int64_t out_bytes, void* workspace, int B, int n, int T, int H, int W, int F,
                                     int K, p4c_stream_t stream) {
    P4C_CHECK_ARG(pred && samples && std && mean && features && spec && params && out && workspace, "p4c_grib_pack_complex: null pointer");
    P4C_CHECK_ARG(B > 0 && n > 0 && n <= GP_MAX_SAMPLES && T > 0 && H > 0 && W > 0 && F > 0 && (int64_t)n * T <= 65535,
                  "p4c_grib_pack_complex: bad dims (B=%d n=%d T=%d H=%d W=%d F=%d; n <= %d, n*T <= 65535)", B, n, T, H, W, F,
                  GP_MAX_SAMPLES);
    P4C_CHECK_ARG(K > 0 && K <= GP_MAX_FEATURES, "p4c_grib_pack_complex: %d features: 1 .. at most %d per call", K, GP_MAX_FEATURES);
    P4C_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                  "p4c_grib_pack_complex: out must be 4-byte aligned, the workspace 16-byte aligned");
    const int64_t N = (int64_t)H * W;
    P4C_CHECK_ARG(N < ((int64_t)1 << 31), "p4c_grib_pack_complex: %lld grid points: at most 2^31 - 1", (long long)N);
    GpSpec sp;
    GcOrder od;
    for (int k = 0; k < K; ++k) {
        const int D = spec[3 * k], nbits = spec[3 * k + 1], order = spec[3 * k + 2];
        P4C_CHECK_ARG(D >= -GP_MAX_D && D <= GP_MAX_D && nbits >= 1 && nbits <= 32,
                      "p4c_grib_pack_complex: spec %d: D = %d, nbits = %d (|D| <= %d and 1 <= nbits <= 32)", k, D, nbits, GP_MAX_D);
        P4C_CHECK_ARG(order >= 0 && order <= 2, "p4c_grib_pack_complex: spec %d: order %d of the spatial differencing: 0 .. 2", k, order);
        P4C_CHECK_ARG(order == 0 || nbits + order <= 31,
                      "p4c_grib_pack_complex: spec %d: nbits = %d at order %d: nbits + order <= 31 fits the descriptors", k, nbits, order);
        sp.d[k] = (int8_t)D;
        sp.nbits[k] = (uint8_t)nbits;
        od.o[k] = (uint8_t)order;
    }
    for (int k = K; k < GP_MAX_FEATURES; ++k) {
        sp.d[k] = 0;
        sp.nbits[k] = 8;
        od.o[k] = 0;
    }
    const int64_t capacity = p4c_grib_pack_complex_capacity(n, T, N, spec, K);
    P4C_CHECK_ARG(capacity < ((int64_t)1 << 31), "p4c_grib_pack_complex: %lld payload bytes in the worst case: at most 2^31 - 1 per call",
                  (long long)capacity);
    P4C_CHECK_ARG(out_bytes >= capacity, "p4c_grib_pack_complex: a buffer of %lld bytes for a capacity of %lld", (long long)out_bytes,
                  (long long)capacity);
    GpSamples smp;
    for (int i = 0; i < n; ++i) {
        P4C_CHECK_ARG(samples[i] >= 0 && samples[i] < B, "p4c_grib_pack_complex: sample %d of a batch of %d", (int)samples[i], B);
        smp.b[i] = samples[i];
    }
    for (int i = n; i < GP_MAX_SAMPLES; ++i) smp.b[i] = 0;
    const bool dense = grib_dense(K, F);
    const int nb = grib_blocks_per_field_set(n, T, N);
    const int ng = (int)gc_groups(N);
    const int64_t fields = (int64_t)n * T * K;
    P4C_CHECK_ARG(fields < ((int64_t)1 << 31), "p4c_grib_pack_complex: %lld fields: fewer than 2^31 per call", (long long)fields);
    const dim3 grid((unsigned)nb, (unsigned)(n * T)), block(GP_THREADS);
    hipStream_t st = as_stream(stream);
    float* partial = (float*)workspace;
    const size_t partial_bytes = (size_t)n * (size_t)T * (size_t)nb * (size_t)K * 3 * sizeof(float);
    GcGroup* groups = (GcGroup*)((char*)workspace + gc_align16(partial_bytes));
    uint32_t* gstart = (uint32_t*)(groups + (size_t)fields * (size_t)ng);
    const bool stored = gc_stored(dense);
    uint32_t* dws = (uint32_t*)((char*)gstart + gc_align16((size_t)fields * (size_t)ng * sizeof(uint32_t)));
    const int64_t dpitch = (int64_t)gc_dpitch(N);
    const int flip = flip_rows ? 1 : 0;
    if (dense)
        hipLaunchKernelGGL(grib_range_kernel<true>, grid, block, 0, st, pred, pred_bs, pred_ts, smp, std, mean, features, partial, T, N, F, K);
    else
        hipLaunchKernelGGL(grib_range_kernel<false>, grid, block, 0, st, pred, pred_bs, pred_ts, smp, std, mean, features, partial, T, N, F, K);
    P4C_CHECK_LAUNCH("p4c_grib_pack_complex(range)");
    hipLaunchKernelGGL(grib_finish_kernel<GC_PARAMS>, dim3((unsigned)K, (unsigned)(n * T)), dim3(64), 0, st, (const float*)partial, sp, params,
                       nb, K);
    P4C_CHECK_LAUNCH("p4c_grib_pack_complex(finish)");
#define P4C_CPX_TILE(DENSE_, PACK_, STORED_)                                                                                            \
    hipLaunchKernelGGL((grib_cpx_tile_kernel<DENSE_, PACK_, STORED_>), grid, block, 0, st, pred, pred_bs, pred_ts, smp, std, mean,     \
                       features, sp, od, params, groups, (const uint32_t*)gstart, out, dws, dpitch, flip, T, (int)N, F, K, H, W, ng)
    if (dense && stored) P4C_CPX_TILE(true, false, true);
    else if (dense) P4C_CPX_TILE(true, false, false);
    else if (stored) P4C_CPX_TILE(false, false, true);
    else P4C_CPX_TILE(false, false, false);
    P4C_CHECK_LAUNCH("p4c_grib_pack_complex(group)");
    hipLaunchKernelGGL(grib_cpx_scan_kernel, dim3((unsigned)fields), dim3(GC_SCAN_THREADS), 0, st, od, params, groups, gstart, (int)N, K, ng);
    P4C_CHECK_LAUNCH("p4c_grib_pack_complex(scan)");
    hipLaunchKernelGGL(grib_cpx_offsets_kernel, dim3(1), dim3(GC_SCAN_THREADS), 0, st, params, fields);
    P4C_CHECK_LAUNCH("p4c_grib_pack_complex(offsets)");
    hipLaunchKernelGGL(grib_cpx_tables_kernel, dim3((unsigned)fields), dim3(GC_SCAN_THREADS), 0, st, od, (const int32_t*)params,
                       (const GcGroup*)groups, out, K, ng);
    P4C_CHECK_LAUNCH("p4c_grib_pack_complex(tables)");
    if (dense && stored) P4C_CPX_TILE(true, true, true);
    else if (dense) P4C_CPX_TILE(true, true, false);
    else if (stored) P4C_CPX_TILE(false, true, true);
    else P4C_CPX_TILE(false, true, false);
#undef P4C_CPX_TILE
    P4C_CHECK_LAUNCH("p4c_grib_pack_complex(pack)");
    return P4C_OK;
}
