// GRIB2 complex packing (data representation templates 5.2 and 5.3: general group splitting, no missing-value management, spatial
// differencing of order 1 or 2) decoded on the device, beside grib_unpack.hip (template 5.0).  The section-7 payloads and the bitmaps
// of a batch lie in one device byte buffer as they are on disk; the host keeps the headers (py4cast_amd/grib2.py: complex_field_of).
//
//   p4c_grib_unpack_complex   `nfields` fields of any sizes (p4c_grib_cfield, include/py4cast_hip.h) -> planes and a status per field.
//
// One field -- the contract grib2.unpack_fields restates in numpy.  The payload holds, each zero-padded to an octet: the descriptors
// (5.3: ival1, ival2 at order 2, gmin, which the HOST parses into the record), ng group references of ref_bits bits, ng widths of
// w_bits bits, ng scaled lengths of l_bits bits, the values in group order.
//   width[g] = w_ref + w[g];   len[g] = l_ref + l_inc * l[g], len[ng-1] = l_last;   a table of 0 bits is absent and all 0;
//   X[k]     = ref[g] + the width[g]-bit integer of value k, which lies in group g (0 at width 0);
//   f        = X (5.2);   f[0] = ival1, f[k] = f[k-1] + X[k] + gmin (order 1);   f[0] = ival1, f[1] = ival2,
//              f[k] = X[k] + gmin + 2 f[k-1] - f[k-2] (order 2): modulo 2^64, read as signed;
//   value    = float( (R + ldexp((double)f, E)) / 10^D )  (D >= 0;  * 10^-D otherwise): float64, every operation a single rounded one
//              (built with -ffp-contract=off);
//   the k-th present point of the bitmap takes value k;  NaN where a point is absent or its rank is >= count;
//   status   1: the lengths do not sum to count;  2: a width above 32;  4: the values end past the stream.  Such a field is all NaN.
//
// The integrations are prefix sums.  With d[j] = X[j] + gmin for j >= order and 0 before, S0(k) = sum of d[j] and S1(k) = sum of
// j * d[j] over j <= k:   order 1: f[k] = ival1 + S0(k);   order 2: f[k] = ival2 + (k-1)(ival2-ival1) + (k+1) S0(k) - S1(k).
//
// A chunk is GC_CHUNK consecutive groups of ONE field, a tile GC_TILE consecutive values (and stream points) of one field.  A
// workgroup takes ceil(n / GC_MAX_BLOCKS) consecutive chunks or tiles of the call and finds their field by bisection, as in
// grib_unpack.hip.  Workgroups depend on each other through launch boundaries only:
//   sums     per chunk: the sums of len and of len * width, and whether a width is above 32;
//   scan     per chunk: the sums of the field's earlier chunks, then an exclusive scan: the first value and the first bit of every
//            group -> workspace; the first chunk of a field adds up all of them and writes the field's status;
//   tiles    (only with an order >= 1 or a bitmap in the call) per tile: (sum d, sum j d) of its values; the population of its bitmap;
//   decode   per tile: a lane owns 8 consecutive values, finds the group of the first by bisection over the groups' first values and
//            walks on from there; the sums of the field's earlier tiles (carried from tile to tile inside a workgroup), a scan of
//            the pair over the 256 lanes, the conversion, and the plane -- or, with a bitmap, the field's value array in `workspace`;
//   scatter  (only with a bitmap in the call) per tile of stream points: ranks from the populations, plane <- value array.
// No atomics, integer sums only: two calls give the same bits.  Every read of a stream goes through gc_word, which reads nothing
// outside [stream_off, stream_off + stream_len) whatever the bytes hold; every store is guarded by its index in the plane.
#include <math.h>

#include "common.hpp"

namespace p4c {

constexpr int GC_THREADS = 256;
constexpr int GC_TILE = 2048;            // values of a tile: 8 per lane
constexpr int GC_PER_LANE = 4;           // groups of a lane in the chunk launches
constexpr int GC_CHUNK = GC_PER_LANE * GC_THREADS;
constexpr int GC_MAX_BLOCKS = 1024;      // workgroups of one launch
constexpr int GC_MAX_D = 15;
constexpr int64_t GC_SATURATE = (int64_t)1 << 40;   // a chunk's sums stop here: far above any field that decodes (2^31 values of 32 bits)
static_assert(GC_TILE == 8 * GC_THREADS, "a lane owns one bitmap octet");

__constant__ double gc_pow10[GC_MAX_D + 1] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};

// where the parts of the workspace lie
struct GcWorkspace {
    int64_t* csum;       // chunks x 3: sum of len, sum of len * width, flags
    int64_t* gbit;       // chunks x GC_CHUNK: the first bit of a group, counted from the first value bit
    uint64_t* tsum;      // tiles x 2: sum of d, sum of j d
    uint32_t* gstart;    // chunks x GC_CHUNK: the first value of a group
    uint32_t* counts;    // tiles: population of the tile's bitmap
    float* vals;         // tiles x GC_TILE: the values of fields with a bitmap, in rank order
};

__host__ __device__ static inline size_t gc_workspace(GcWorkspace& w, void* base, int64_t tiles, int64_t chunks, bool bitmap) {
    char* p = (char*)base;
    size_t at = 0;
    w.csum = (int64_t*)(p + at);
    at += (size_t)chunks * 3 * sizeof(int64_t);
    w.gbit = (int64_t*)(p + at);
    at += (size_t)chunks * GC_CHUNK * sizeof(int64_t);
    w.tsum = (uint64_t*)(p + at);
    at += (size_t)tiles * 2 * sizeof(uint64_t);
    w.gstart = (uint32_t*)(p + at);
    at += (size_t)chunks * GC_CHUNK * sizeof(uint32_t);
    w.counts = (uint32_t*)(p + at);
    at += (size_t)tiles * sizeof(uint32_t);
    w.vals = (float*)(p + at);
    if (bitmap) at += (size_t)tiles * GC_TILE * sizeof(float);
    return at;
}

// octets of the descriptors in front of the tables
__host__ __device__ static inline int64_t gc_descriptor_bytes(const p4c_grib_cfield& f) {
    return f.order > 0 ? (int64_t)(f.order + 1) * f.nbytes : 0;
}

// the first bit of the references, the widths, the lengths and the values
struct GcBits {
    int64_t ref, width, len, values;
};

__host__ __device__ static inline GcBits gc_bits_of(const p4c_grib_cfield& f) {
    GcBits b;
    const int64_t ng = f.ng;
    b.ref = 8 * gc_descriptor_bytes(f);
    b.width = b.ref + 8 * ((ng * f.ref_bits + 7) / 8);
    b.len = b.width + 8 * ((ng * f.w_bits + 7) / 8);
    b.values = b.len + 8 * ((ng * f.l_bits + 7) / 8);
    return b;
}

// word i of a stream of `len` bytes as the big-endian number it is in the file; bytes past the end read as 0 and are not touched
__device__ __forceinline__ uint32_t gc_word(const unsigned char* __restrict__ s, int64_t i, int64_t len) {
    if (i < 0 || i > (len >> 2)) return 0u;
    const int64_t at = 4 * i;
    if (at + 4 <= len) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(s + at));
    uint32_t w = 0u;
    for (int j = 0; j < 4; ++j)
        if (at + j < len) w |= (uint32_t)s[at + j] << (24 - 8 * j);
    return w;
}

// the n-bit integer (1 <= n <= 32) at bit `bit` of the stream, most significant bit first
__device__ __forceinline__ uint32_t gc_bits(const unsigned char* __restrict__ s, int64_t len, int64_t bit, int n) {
    const int64_t wi = bit >> 5;
    const int sh = (int)(bit & 31);
    const uint32_t hi = gc_word(s, wi, len);
    const uint32_t lo = sh + n > 32 ? gc_word(s, wi + 1, len) : 0u;
    const uint64_t window = ((uint64_t)hi << 32) | lo;
    return (uint32_t)((window << sh) >> (64 - n));
}

__device__ __forceinline__ uint64_t gc_shfl_up(uint64_t v, int o) {
    const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t gc_shfl_xor(uint64_t v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

// the sum of v over the workgroup, in every lane.  Every lane of the workgroup calls it.
__device__ __forceinline__ uint64_t gc_block_sum(uint64_t v, uint64_t* slots) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += gc_shfl_xor(v, o);
    __syncthreads();   // earlier readers of the slots are done
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    return slots[0] + slots[1] + slots[2] + slots[3];
}

// the sum of v over the lanes before this one; `total` over all of them.  Every lane of the workgroup calls it.
__device__ __forceinline__ uint64_t gc_block_exclusive(uint64_t v, uint64_t* slots, uint64_t& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = gc_shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) slots[wv] = inc;
    __syncthreads();
    uint64_t upto = 0;
    for (int w = 0; w < wv; ++w) upto += slots[w];
    total = slots[0] + slots[1] + slots[2] + slots[3];
    return upto + inc - v;
}

// the field of a tile / of a chunk: the last one whose first is not past it (both grow strictly: every field has one at least)
template <bool CHUNKS>
__device__ __forceinline__ int gc_first_of(const p4c_grib_cfield& f) {
    return CHUNKS ? f.chunk0 : f.tile0;
}

template <bool CHUNKS>
__device__ __forceinline__ int gc_field_of(const p4c_grib_cfield* __restrict__ fields, int nfields, int item) {
    int lo = 0, hi = nfields - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (gc_first_of<CHUNKS>(fields[mid]) <= item)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

template <bool CHUNKS>
__device__ __forceinline__ int gc_next0(const p4c_grib_cfield* __restrict__ fields, int nfields, int fi, int items) {
    return fi + 1 < nfields ? gc_first_of<CHUNKS>(fields[fi + 1]) : items;
}

// length and width of group g; a length above count counts as count + 1 (the sum is wrong either way), a width above 32 as 0
__device__ __forceinline__ void gc_group(const p4c_grib_cfield& f, const GcBits& b, const unsigned char* __restrict__ sp, int64_t g,
                                         int64_t& len, int& width, int& flags) {
    const uint32_t w = f.w_bits > 0 ? gc_bits(sp, f.stream_len, b.width + g * f.w_bits, f.w_bits) : 0u;
    const uint32_t l = f.l_bits > 0 ? gc_bits(sp, f.stream_len, b.len + g * f.l_bits, f.l_bits) : 0u;
    const int64_t wd = (int64_t)f.w_ref + w;
    width = (int)wd;
    if (wd > 32) {
        flags |= 2;
        width = 0;
    }
    len = g == (int64_t)f.ng - 1 ? (int64_t)f.l_last : (int64_t)f.l_ref + (int64_t)f.l_inc * l;
    if (len > f.count) len = (int64_t)f.count + 1;
}

// launch 1.  csum[chunk] = (sum of len, sum of len * width, flags) over the groups of the chunk
__global__ void __launch_bounds__(GC_THREADS)
    grib_complex_sums_kernel(const unsigned char* __restrict__ bytes, const p4c_grib_cfield* __restrict__ fields, int nfields,
                             GcWorkspace ws, int chunks, int per) {
    __shared__ uint64_t slots[GC_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * per;
    const int end = first + per < chunks ? (int)(first + per) : chunks;
    if (first >= end) return;
    int fi = gc_field_of<true>(fields, nfields, (int)first);
    int next0 = gc_next0<true>(fields, nfields, fi, chunks);
    p4c_grib_cfield f = fields[fi];
    for (int chunk = (int)first; chunk < end; ++chunk) {
        if (chunk >= next0) {
            f = fields[++fi];
            next0 = gc_next0<true>(fields, nfields, fi, chunks);
        }
        const GcBits b = gc_bits_of(f);
        const unsigned char* __restrict__ sp = bytes + f.stream_off;
        const int64_t g0 = (int64_t)(chunk - f.chunk0) * GC_CHUNK + tid * GC_PER_LANE;
        uint64_t lens = 0, bits = 0;
        int flags = 0;
        for (int j = 0; j < GC_PER_LANE; ++j) {
            if (g0 + j >= (int64_t)f.ng) break;
            int64_t len;
            int width;
            gc_group(f, b, sp, g0 + j, len, width, flags);
            lens += (uint64_t)len;
            bits += (uint64_t)(len * width);
        }
        lens = gc_block_sum(lens, slots);
        bits = gc_block_sum(bits, slots);
        const uint64_t any = gc_block_sum((uint64_t)(flags != 0), slots);
        if (tid == 0) {
            ws.csum[3 * (int64_t)chunk] = (int64_t)lens < GC_SATURATE ? (int64_t)lens : GC_SATURATE;
            ws.csum[3 * (int64_t)chunk + 1] = (int64_t)bits < GC_SATURATE ? (int64_t)bits : GC_SATURATE;
            ws.csum[3 * (int64_t)chunk + 2] = any ? 2 : 0;
        }
    }
}

// launch 2.  The first value and the first bit of every group; the first chunk of a field writes the field's status
__global__ void __launch_bounds__(GC_THREADS)
    grib_complex_scan_kernel(const unsigned char* __restrict__ bytes, const p4c_grib_cfield* __restrict__ fields, int nfields,
                             GcWorkspace ws, int32_t* __restrict__ status, int chunks, int per) {
    __shared__ uint64_t slots[GC_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * per;
    const int end = first + per < chunks ? (int)(first + per) : chunks;
    if (first >= end) return;
    int fi = gc_field_of<true>(fields, nfields, (int)first);
    int next0 = gc_next0<true>(fields, nfields, fi, chunks);
    p4c_grib_cfield f = fields[fi];
    for (int chunk = (int)first; chunk < end; ++chunk) {
        if (chunk >= next0) {
            f = fields[++fi];
            next0 = gc_next0<true>(fields, nfields, fi, chunks);
        }
        const GcBits b = gc_bits_of(f);
        const unsigned char* __restrict__ sp = bytes + f.stream_off;
        const int c = chunk - f.chunk0;
        // the chunks before this one; for the first chunk of the field, all of them: the field's totals
        const int upto = c == 0 ? next0 - f.chunk0 : c;
        uint64_t lens = 0, bits = 0, any = 0;
        for (int i = tid; i < upto; i += GC_THREADS) {
            const int64_t* s = ws.csum + 3 * (int64_t)(f.chunk0 + i);
            lens += (uint64_t)s[0];
            bits += (uint64_t)s[1];
            any |= (uint64_t)s[2];
        }
        lens = gc_block_sum(lens, slots);
        bits = gc_block_sum(bits, slots);
        any = gc_block_sum(any, slots);
        if (c == 0) {
            if (tid == 0) {
                int st = any ? 2 : 0;
                if ((int64_t)lens != (int64_t)f.count) st |= 1;
                if (b.values + (int64_t)bits > 8 * f.stream_len) st |= 4;
                status[fi] = st;
            }
            lens = 0;
            bits = 0;
        }
        const int64_t g0 = (int64_t)c * GC_CHUNK + tid * GC_PER_LANE;
        int64_t len[GC_PER_LANE];
        int width[GC_PER_LANE];
        uint64_t mine_len = 0, mine_bits = 0;
        int flags = 0;
#pragma unroll
        for (int j = 0; j < GC_PER_LANE; ++j) {
            len[j] = 0;
            width[j] = 0;
            if (g0 + j < (int64_t)f.ng) gc_group(f, b, sp, g0 + j, len[j], width[j], flags);
            mine_len += (uint64_t)len[j];
            mine_bits += (uint64_t)(len[j] * width[j]);
        }
        uint64_t total;
        uint64_t at_len = lens + gc_block_exclusive(mine_len, slots, total);
        uint64_t at_bit = bits + gc_block_exclusive(mine_bits, slots, total);
        const int64_t slot0 = (int64_t)chunk * GC_CHUNK + tid * GC_PER_LANE;
#pragma unroll
        for (int j = 0; j < GC_PER_LANE; ++j) {
            if (g0 + j < (int64_t)f.ng) {
                ws.gstart[slot0 + j] = at_len < 0xffffffffull ? (uint32_t)at_len : 0xffffffffu;
                ws.gbit[slot0 + j] = (int64_t)at_bit;
            }
            at_len += (uint64_t)len[j];
            at_bit += (uint64_t)(len[j] * width[j]);
        }
    }
}

// the presence bits of the 8 points from p0 on, point i in bit 7 - i; `valid` of them exist
__device__ __forceinline__ uint32_t gc_presence(const unsigned char* __restrict__ bitmap, int p0, int valid) {
    if (valid <= 0) return 0u;
    const uint32_t m = bitmap[p0 >> 3];
    return valid < 8 ? m & (0xff00u >> valid) & 0xffu : m;
}

// the last group of [lo, ng) whose first value is not past k; gstart[lo] <= k
__device__ __forceinline__ int64_t gc_group_of(const uint32_t* __restrict__ gstart, int64_t lo, int64_t ng, uint32_t k) {
    int64_t hi = ng - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (gstart[mid] <= k)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// d[i] of the 8 values from k0 on (0 for a value past count): X for 5.2, X + gmin from value `order` on and 0 before for 5.3.
// The field's status is 0: the lengths sum to count, so every value below count lies in a group.
__device__ __forceinline__ void gc_extract(uint64_t (&d)[8], const p4c_grib_cfield& f, const GcBits& b,
                                           const unsigned char* __restrict__ sp, const GcWorkspace& ws, int64_t k0) {
    const uint32_t* __restrict__ gstart = ws.gstart + (int64_t)f.chunk0 * GC_CHUNK;
    const int64_t* __restrict__ gbit = ws.gbit + (int64_t)f.chunk0 * GC_CHUNK;
    const int64_t ng = f.ng;
    int64_t g = -1, g_first = 0, g_end = 0, g_bit = 0;
    uint64_t ref = 0;
    int width = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        d[i] = 0;
        const int64_t k = k0 + i;
        if (k >= f.count) continue;
        if (g < 0 || k >= g_end) {
            g = gc_group_of(gstart, g < 0 ? 0 : g, ng, (uint32_t)k);
            g_first = gstart[g];
            g_end = g + 1 < ng ? (int64_t)gstart[g + 1] : (int64_t)f.count;
            g_bit = gbit[g];
            int64_t len;
            int flags = 0;
            gc_group(f, b, sp, g, len, width, flags);
            ref = f.ref_bits > 0 ? gc_bits(sp, f.stream_len, b.ref + g * f.ref_bits, f.ref_bits) : 0u;
        }
        const uint64_t v = width > 0 ? gc_bits(sp, f.stream_len, b.values + g_bit + (k - g_first) * width, width) : 0u;
        const uint64_t X = ref + v;
        d[i] = f.order == 0 ? X : k < f.order ? 0ull : X + (uint64_t)f.gmin;
    }
}

// launch 3.  Per tile: (sum of d, sum of j d) where the field is differenced, the population of the bitmap where it has one
__global__ void __launch_bounds__(GC_THREADS)
    grib_complex_tiles_kernel(const unsigned char* __restrict__ bytes, const p4c_grib_cfield* __restrict__ fields, int nfields,
                              GcWorkspace ws, const int32_t* __restrict__ status, int tiles, int per) {
    __shared__ uint64_t slots[GC_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * per;
    const int end = first + per < tiles ? (int)(first + per) : tiles;
    if (first >= end) return;
    int fi = gc_field_of<false>(fields, nfields, (int)first);
    int next0 = gc_next0<false>(fields, nfields, fi, tiles);
    p4c_grib_cfield f = fields[fi];
    int st = status[fi];
    for (int tile = (int)first; tile < end; ++tile) {
        if (tile >= next0) {
            f = fields[++fi];
            st = status[fi];
            next0 = gc_next0<false>(fields, nfields, fi, tiles);
        }
        const int N = f.ni * f.nj;
        const int64_t k0 = (int64_t)(tile - f.tile0) * GC_TILE + tid * 8;
        if (f.bitmap_off >= 0) {
            const int valid = N - k0 < 8 ? (int)(N - k0) : 8;
            const uint64_t n = gc_block_sum((uint64_t)__popc(gc_presence(bytes + f.bitmap_off, (int)k0, valid)), slots);
            if (tid == 0) ws.counts[tile] = (uint32_t)n;
        }
        if (f.order > 0 && st == 0) {
            const GcBits b = gc_bits_of(f);
            uint64_t d[8], s0 = 0, s1 = 0;
            gc_extract(d, f, b, bytes + f.stream_off, ws, k0);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                s0 += d[i];
                s1 += (uint64_t)(k0 + i) * d[i];
            }
            s0 = gc_block_sum(s0, slots);
            s1 = gc_block_sum(s1, slots);
            if (tid == 0) {
                ws.tsum[2 * (int64_t)tile] = s0;
                ws.tsum[2 * (int64_t)tile + 1] = s1;
            }
        }
    }
}

__device__ __forceinline__ float gc_value(uint64_t fv, double R, int E, int D, double pw) {
    const double t = R + ldexp((double)(int64_t)fv, E);
    const double y = D >= 0 ? t / pw : t * pw;
    return (float)y;
}

// the 8 plane elements of the stream points from p0 on (`valid` of them exist, valid > 0)
__device__ __forceinline__ void gc_store(const float (&out)[8], const p4c_grib_cfield& f, float* __restrict__ plane, int p0, int valid) {
    int r = 0, c = 0;
    bool run = valid == 8;   // 8 consecutive plane elements
    int64_t d0 = p0;
    if (f.flip_rows) {
        r = p0 / f.ni;
        c = p0 - r * f.ni;
        run = run && c + 8 <= f.ni;
        d0 = (int64_t)(f.nj - 1 - r) * f.ni + c;
    }
    if (run && (reinterpret_cast<uintptr_t>(plane + d0) & 15) == 0) {
        float4* d4 = reinterpret_cast<float4*>(plane + d0);
        d4[0] = make_float4(out[0], out[1], out[2], out[3]);
        d4[1] = make_float4(out[4], out[5], out[6], out[7]);
    } else if (!f.flip_rows) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < valid) plane[d0 + i] = out[i];
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < valid) plane[(int64_t)(f.nj - 1 - r) * f.ni + c] = out[i];
            if (++c == f.ni) {
                c = 0;
                ++r;
            }
        }
    }
}

// launch 4.  The values of a tile: into the plane, or with a bitmap into the field's value array
__global__ void __launch_bounds__(GC_THREADS)
    grib_complex_decode_kernel(const unsigned char* __restrict__ bytes, const p4c_grib_cfield* __restrict__ fields, int nfields,
                               float* __restrict__ planes, GcWorkspace ws, const int32_t* __restrict__ status, int tiles, int per) {
    __shared__ uint64_t slots[GC_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * per;
    const int end = first + per < tiles ? (int)(first + per) : tiles;
    if (first >= end) return;
    int fi = gc_field_of<false>(fields, nfields, (int)first);
    int next0 = gc_next0<false>(fields, nfields, fi, tiles);
    p4c_grib_cfield f = fields[fi];
    int st = status[fi];
    bool carried = false;   // (base0, base1) are the sums of the field's tiles before this one: the previous trip's tile was that one
    uint64_t base0 = 0, base1 = 0;
    for (int tile = (int)first; tile < end; ++tile) {
        if (tile >= next0) {
            f = fields[++fi];
            st = status[fi];
            next0 = gc_next0<false>(fields, nfields, fi, tiles);
            carried = false;
        }
        const int N = f.ni * f.nj;
        const int t = tile - f.tile0;
        const int64_t k0 = (int64_t)t * GC_TILE + tid * 8;
        const bool has_bitmap = f.bitmap_off >= 0;
        const int valid = N - k0 < 8 ? (int)(N - k0) : 8;   // points of the lane; <= 0: past the field
        float out[8];
        if (st != 0) {   // the scatter launch fills the plane of a field with a bitmap
            if (!has_bitmap && valid > 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) out[i] = NAN;
                gc_store(out, f, planes + f.dst_off, (int)k0, valid);
            }
            continue;
        }
        const GcBits b = gc_bits_of(f);
        uint64_t d[8];
        gc_extract(d, f, b, bytes + f.stream_off, ws, k0);
        if (f.order > 0) {
            if (!carried) {
                uint64_t s0 = 0, s1 = 0;
                for (int i = tid; i < t; i += GC_THREADS) {
                    s0 += ws.tsum[2 * (int64_t)(f.tile0 + i)];
                    s1 += ws.tsum[2 * (int64_t)(f.tile0 + i) + 1];
                }
                base0 = gc_block_sum(s0, slots);
                base1 = gc_block_sum(s1, slots);
            }
            uint64_t s0 = 0, s1 = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                s0 += d[i];
                s1 += (uint64_t)(k0 + i) * d[i];
            }
            uint64_t total0, total1;
            uint64_t at0 = base0 + gc_block_exclusive(s0, slots, total0);
            uint64_t at1 = base1 + gc_block_exclusive(s1, slots, total1);
            base0 += total0;
            base1 += total1;
            carried = true;
            const uint64_t i1 = (uint64_t)f.ival1, i2 = (uint64_t)f.ival2;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint64_t k = (uint64_t)(k0 + i);
                at0 += d[i];
                at1 += k * d[i];
                d[i] = f.order == 1 ? i1 + at0 : i2 + (k - 1) * (i2 - i1) + (k + 1) * at0 - at1;
            }
        }
        const double R = (double)f.R;
        const double pw = gc_pow10[f.D >= 0 ? f.D : -f.D];
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = k0 + i < f.count ? gc_value(d[i], R, f.E, f.D, pw) : NAN;
        if (!has_bitmap) {
            if (valid > 0) gc_store(out, f, planes + f.dst_off, (int)k0, valid);   // count == N
        } else {
            float* __restrict__ vals = ws.vals + (int64_t)f.tile0 * GC_TILE;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (k0 + i < f.count && i < valid) vals[k0 + i] = out[i];
        }
    }
}

// launch 5.  The planes of the fields with a bitmap: the k-th present point takes value k of the field's value array
__global__ void __launch_bounds__(GC_THREADS)
    grib_complex_scatter_kernel(const unsigned char* __restrict__ bytes, const p4c_grib_cfield* __restrict__ fields, int nfields,
                                float* __restrict__ planes, GcWorkspace ws, const int32_t* __restrict__ status, int tiles, int per) {
    __shared__ uint64_t slots[GC_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * per;
    const int end = first + per < tiles ? (int)(first + per) : tiles;
    if (first >= end) return;
    int fi = gc_field_of<false>(fields, nfields, (int)first);
    int next0 = gc_next0<false>(fields, nfields, fi, tiles);
    p4c_grib_cfield f = fields[fi];
    int st = status[fi];
    bool carried = false;
    uint64_t rank = 0;
    for (int tile = (int)first; tile < end; ++tile) {
        if (tile >= next0) {
            f = fields[++fi];
            st = status[fi];
            next0 = gc_next0<false>(fields, nfields, fi, tiles);
            carried = false;
        }
        if (f.bitmap_off < 0) continue;
        const int N = f.ni * f.nj;
        const int t = tile - f.tile0;
        const int64_t p0 = (int64_t)t * GC_TILE + tid * 8;
        const int valid = N - p0 < 8 ? (int)(N - p0) : 8;
        const uint32_t mask = gc_presence(bytes + f.bitmap_off, (int)p0, valid);
        if (!carried) {
            uint64_t before = 0;
            for (int i = tid; i < t; i += GC_THREADS) before += ws.counts[f.tile0 + i];
            rank = gc_block_sum(before, slots);
        }
        uint64_t total;
        uint64_t k = rank + gc_block_exclusive((uint64_t)__popc(mask), slots, total);
        rank += total;
        carried = true;
        if (valid <= 0) continue;   // after the barriers
        const float* __restrict__ vals = ws.vals + (int64_t)f.tile0 * GC_TILE;
        float out[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            out[i] = NAN;
            if ((mask >> (7 - i)) & 1u) {
                if (st == 0 && k < (uint64_t)f.count) out[i] = vals[k];
                ++k;
            }
        }
        gc_store(out, f, planes + f.dst_off, (int)p0, valid);
    }
}

}  // namespace p4c

using namespace p4c;

extern "C" int p4c_grib_complex_tile(void) { return GC_TILE; }
extern "C" int p4c_grib_complex_chunk(void) { return GC_CHUNK; }
extern "C" int p4c_grib_complex_max_blocks(void) { return GC_MAX_BLOCKS; }
extern "C" size_t p4c_grib_unpack_complex_workspace_bytes(int64_t tiles, int64_t chunks, int has_bitmap) {
    GcWorkspace w;
    return tiles > 0 && chunks > 0 ? gc_workspace(w, nullptr, tiles, chunks, has_bitmap != 0) : 0;
}

extern "C" int p4c_grib_unpack_complex(const unsigned char* bytes, int64_t nbytes, const p4c_grib_cfield* fields,
                                       const p4c_grib_cfield* fields_host, int nfields, float* planes, int32_t* status, void* workspace,
                                       p4c_stream_t stream) {
    const char* me = "p4c_grib_unpack_complex";
    P4C_CHECK_ARG(bytes && fields && fields_host && planes && status && workspace, "%s: null pointer", me);
    P4C_CHECK_ARG((reinterpret_cast<uintptr_t>(bytes) & 3) == 0 && (reinterpret_cast<uintptr_t>(planes) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                  "%s: bytes and planes must be 4-byte aligned, the workspace 8-byte aligned", me);
    P4C_CHECK_ARG(nfields > 0 && nbytes >= 0, "%s: %d fields in %lld bytes", me, nfields, (long long)nbytes);
    int64_t tiles = 0, chunks = 0;
    bool any_bitmap = false, any_order = false;
    for (int i = 0; i < nfields; ++i) {
        const p4c_grib_cfield& f = fields_host[i];
        P4C_CHECK_ARG(f.ni > 0 && f.nj > 0, "%s: field %d: a grid of %d x %d", me, i, f.nj, f.ni);
        const int64_t N = (int64_t)f.ni * f.nj;
        P4C_CHECK_ARG(N < ((int64_t)1 << 31), "%s: field %d: %lld points: at most 2^31 - 1", me, i, (long long)N);
        P4C_CHECK_ARG(f.D >= -GC_MAX_D && f.D <= GC_MAX_D, "%s: field %d: D = %d (|D| <= %d)", me, i, f.D, GC_MAX_D);
        P4C_CHECK_ARG(f.count >= 0 && f.count <= N, "%s: field %d: %d values for %lld points", me, i, f.count, (long long)N);
        P4C_CHECK_ARG(f.bitmap_off >= -1, "%s: field %d: bitmap_off = %lld (-1: no bitmap)", me, i, (long long)f.bitmap_off);
        P4C_CHECK_ARG(f.bitmap_off >= 0 || f.count == N, "%s: field %d: no bitmap and %d values for %lld points", me, i, f.count, (long long)N);
        P4C_CHECK_ARG(f.stream_off >= 0 && (f.stream_off & 3) == 0 && (f.bitmap_off < 0 || (f.bitmap_off & 3) == 0) && f.dst_off >= 0 &&
                          (f.dst_off & 3) == 0,
                      "%s: field %d: stream_off = %lld, bitmap_off = %lld, dst_off = %lld: multiples of 4, not negative", me, i,
                      (long long)f.stream_off, (long long)f.bitmap_off, (long long)f.dst_off);
        P4C_CHECK_ARG(f.ref_bits >= 0 && f.ref_bits <= 32 && f.w_bits >= 0 && f.w_bits <= 32 && f.l_bits >= 0 && f.l_bits <= 32,
                      "%s: field %d: ref_bits = %d, w_bits = %d, l_bits = %d: 0 .. 32 each", me, i, f.ref_bits, f.w_bits, f.l_bits);
        P4C_CHECK_ARG(f.w_ref >= 0 && f.w_ref <= 255 && f.l_inc >= 0 && f.l_inc <= 255, "%s: field %d: w_ref = %d, l_inc = %d: one octet each",
                      me, i, f.w_ref, f.l_inc);
        P4C_CHECK_ARG(f.order >= 0 && f.order <= 2 && f.nbytes >= 0 && f.nbytes <= 4, "%s: field %d: order = %d, nbytes = %d (0 .. 2, 0 .. 4)",
                      me, i, f.order, f.nbytes);
        P4C_CHECK_ARG(f.ng < ((uint32_t)1 << 31), "%s: field %d: %u groups: at most 2^31 - 1", me, i, f.ng);
        P4C_CHECK_ARG(f.ng > 0 || f.count == 0, "%s: field %d: no group for %d values", me, i, f.count);
        P4C_CHECK_ARG(f.stream_len >= 0 && f.stream_len <= (((int64_t)1 << 60) - 1) / 8 && f.stream_len >= gc_bits_of(f).values / 8,
                      "%s: field %d: a stream of %lld bytes for %lld bytes of descriptors and group tables", me, i, (long long)f.stream_len,
                      (long long)(gc_bits_of(f).values / 8));
        P4C_CHECK_ARG(f.stream_off <= nbytes && f.stream_len <= nbytes - f.stream_off, "%s: field %d: the stream [%lld, +%lld) leaves the %lld bytes",
                      me, i, (long long)f.stream_off, (long long)f.stream_len, (long long)nbytes);
        P4C_CHECK_ARG(f.bitmap_off < 0 || (f.bitmap_off <= nbytes && (N + 7) / 8 <= nbytes - f.bitmap_off),
                      "%s: field %d: the bitmap [%lld, +%lld) leaves the %lld bytes", me, i, (long long)f.bitmap_off, (long long)((N + 7) / 8),
                      (long long)nbytes);
        P4C_CHECK_ARG(f.tile0 == tiles && f.chunk0 == chunks, "%s: field %d: tile0 = %d, chunk0 = %d, the tiles and chunks before it are %lld, %lld",
                      me, i, f.tile0, f.chunk0, (long long)tiles, (long long)chunks);
        tiles += (N + GC_TILE - 1) / GC_TILE;
        chunks += f.ng > 0 ? ((int64_t)f.ng + GC_CHUNK - 1) / GC_CHUNK : 1;
        P4C_CHECK_ARG(tiles < ((int64_t)1 << 31) && chunks < ((int64_t)1 << 31), "%s: %lld tiles, %lld chunks: at most 2^31 - 1 per call", me,
                      (long long)tiles, (long long)chunks);
        any_bitmap = any_bitmap || f.bitmap_off >= 0;
        any_order = any_order || f.order > 0;
    }
    GcWorkspace ws;
    gc_workspace(ws, workspace, tiles, chunks, any_bitmap);
    hipStream_t st = as_stream(stream);
    const int per_c = (int)((chunks + GC_MAX_BLOCKS - 1) / GC_MAX_BLOCKS);
    const unsigned blocks_c = (unsigned)((chunks + per_c - 1) / per_c);
    const int per_t = (int)((tiles + GC_MAX_BLOCKS - 1) / GC_MAX_BLOCKS);
    const unsigned blocks_t = (unsigned)((tiles + per_t - 1) / per_t);
    hipLaunchKernelGGL(grib_complex_sums_kernel, dim3(blocks_c), dim3(GC_THREADS), 0, st, bytes, fields, nfields, ws, (int)chunks, per_c);
    P4C_CHECK_LAUNCH("p4c_grib_unpack_complex(sums)");
    hipLaunchKernelGGL(grib_complex_scan_kernel, dim3(blocks_c), dim3(GC_THREADS), 0, st, bytes, fields, nfields, ws, status, (int)chunks, per_c);
    P4C_CHECK_LAUNCH("p4c_grib_unpack_complex(scan)");
    if (any_order || any_bitmap) {
        hipLaunchKernelGGL(grib_complex_tiles_kernel, dim3(blocks_t), dim3(GC_THREADS), 0, st, bytes, fields, nfields, ws,
                           (const int32_t*)status, (int)tiles, per_t);
        P4C_CHECK_LAUNCH("p4c_grib_unpack_complex(tiles)");
    }
    hipLaunchKernelGGL(grib_complex_decode_kernel, dim3(blocks_t), dim3(GC_THREADS), 0, st, bytes, fields, nfields, planes, ws,
                       (const int32_t*)status, (int)tiles, per_t);
    P4C_CHECK_LAUNCH("p4c_grib_unpack_complex(decode)");
    if (any_bitmap) {
        hipLaunchKernelGGL(grib_complex_scatter_kernel, dim3(blocks_t), dim3(GC_THREADS), 0, st, bytes, fields, nfields, planes, ws,
                           (const int32_t*)status, (int)tiles, per_t);
        P4C_CHECK_LAUNCH("p4c_grib_unpack_complex(scatter)");
    }
    return P4C_OK;
}
