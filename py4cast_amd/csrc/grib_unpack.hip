// GRIB2 simple packing (data representation template 5.0) decoded on the device: the read side of grib_pack.hip.  The reference's
// Titan accessor reads GRIB by default (datasets/titan/__init__.py:112-152, 211-226: cfgrib / eccodes decode every field on the
// host and the fp32 planes cross to the device afterwards); here the packed bit streams and bitmaps of a whole batch are copied as
// they lie in the files and unpacked into the fp32 planes datapipe.load_native_batch consumes.  The host keeps the headers
// (py4cast_amd/grib2.py: field_of).
//
//   p4c_grib_unpack   `nfields` fields of any sizes (p4c_grib_field, include/py4cast_hip.h) -> planes.
//
// One field of N = ni*nj stream points -- the contract grib2.unpack_fields restates in numpy:
//   present(p)  no bitmap, or bit 7 - p%8 of bitmap octet p/8;
//   rank(p)     the number of present points before p;
//   X           the nbits-bit big-endian integer at bit rank(p)*nbits of the stream (0 for nbits == 0);
//   value       float( (R + ldexp(X, E)) / 10^D )  (D >= 0;  * 10^-D otherwise): float64, every operation a single rounded one
//               (built with -ffp-contract=off; 10^|D| is exact for |D| <= 15);
//   NaN         where p is absent or rank(p) >= count;
//   plane element (p / ni, p % ni), or (nj-1 - p/ni, p % ni) with flip_rows.
//
// A tile is GU_TILE consecutive stream points of ONE field.  A workgroup takes `per` = ceil(tiles / GU_MAX_BLOCKS) CONSECUTIVE tiles
// of the call: it finds the field of its first tile by bisection over the tile0 column of the table and moves on to the next
// field when its tiles run out.
//   count    (only when a field has a bitmap) a wave owns a tile, a lane one 32-bit word of its bitmap: workspace[tile] = the
//            population of the tile.  No barrier.
//   unpack   a lane owns 8 points: one bitmap octet, 32 output bytes (two 16-byte stores when they stay in one plane row), and --
//            without a bitmap -- nbits whole stream octets, which it walks through a 64-bit window of byte-swapped words, loading
//            one new word when the window moves on.  16 bits without a bitmap (what operational files and ForecastGribWriter
//            mostly hold): one 16-byte load, 8 values.
//            With a bitmap the rank of a tile's first point is the sum of workspace[tile0 .. tile) for the first tile of the
//            workgroup (at most N / GU_TILE values, a few hundred for an AROME grid) and carried on from tile to tile after
//            that; the octets' populations are scanned over the 256 lanes.  The values of a tile are ONE piece of the stream, which
//            the workgroup stages in LDS with coalesced word loads, byte-swapped; the lanes' windows read LDS.
// No atomics, integer sums only: two calls give the same bits.  No byte outside a field's stream and bitmap is read: the last,
// partial word of a stream is put together from its bytes.
#include <math.h>

#include "common.hpp"

namespace p4c {

constexpr int GU_TILE = 2048;            // points per loop trip of a workgroup: 8 per lane
constexpr int GU_THREADS = 256;
constexpr int GU_MAX_BLOCKS = 2048;      // workgroups of one launch
constexpr int GU_MAX_D = 15;
static_assert(GU_TILE == 8 * GU_THREADS, "a lane owns one bitmap octet");
static_assert(GU_TILE == 32 * 64, "in the count launch a wave owns a tile, a lane one word of its bitmap");
// words of a tile's piece of a stream: GU_TILE values of 32 bits that start inside a word, and the window's second word
constexpr int GU_STAGE = GU_TILE + 4;

// 16 bytes at 4-byte alignment: stream_off is a multiple of 4 in a buffer the caller aligned to 4 bytes
struct __attribute__((aligned(4))) GuWords4 {
    uint32_t w[4];
};

__constant__ double gu_pow10[GU_MAX_D + 1] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};

__host__ __device__ static inline bool gu_fast(int nbits, bool has_bitmap) { return nbits == 16 && !has_bitmap; }

// the field of a tile: the last one whose tile0 is not past it (tile0 grows strictly: every field has at least one tile)
__device__ __forceinline__ int gu_field_of(const p4c_grib_field* __restrict__ fields, int nfields, int tile) {
    int lo = 0, hi = nfields - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (fields[mid].tile0 <= tile)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// the presence bits of the 8 points from p0 on, point i in bit 7 - i; `valid` of them exist
__device__ __forceinline__ uint32_t gu_presence(const unsigned char* __restrict__ bitmap, int p0, int valid) {
    if (valid <= 0) return 0u;
    const uint32_t m = bitmap[p0 >> 3];
    return valid < 8 ? m & (0xff00u >> valid) & 0xffu : m;
}

// word i of a stream of `len` bytes as the big-endian number it is in the file; bytes past the end read as 0 and are not touched
__device__ __forceinline__ uint32_t gu_word(const unsigned char* __restrict__ s, int64_t i, int64_t len) {
    const int64_t at = 4 * i;
    if (at + 4 <= len) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(s + at));
    uint32_t w = 0u;
    for (int j = 0; j < 4; ++j)
        if (at + j < len) w |= (uint32_t)s[at + j] << (24 - 8 * j);
    return w;
}

__device__ __forceinline__ float gu_value(uint32_t X, double R, int E, int D, double pw) {
    const double t = R + ldexp((double)X, E);
    const double y = D >= 0 ? t / pw : t * pw;
    return (float)y;
}

// the field after `fi` starts at this tile (the end of the call after the last field)
__device__ __forceinline__ int gu_next0(const p4c_grib_field* __restrict__ fields, int nfields, int fi, int tiles) {
    return fi + 1 < nfields ? fields[fi + 1].tile0 : tiles;
}

// workgroup b takes the tiles [b*per, (b+1)*per), its waves one tile each in turn; a lane counts 32 points: one word of the bitmap.
// workspace[tile] = the number of present points of the tile (tiles of fields without a bitmap: not written).  No barrier.
__global__ void __launch_bounds__(GU_THREADS)
    grib_count_kernel(const unsigned char* __restrict__ bytes, const p4c_grib_field* __restrict__ fields, int nfields,
                      uint32_t* __restrict__ counts, int tiles, int per) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t first = (int64_t)blockIdx.x * per + wv;
    const int end = (int64_t)(blockIdx.x + 1) * per < tiles ? (int)((int64_t)(blockIdx.x + 1) * per) : tiles;
    if (first >= end) return;
    int fi = gu_field_of(fields, nfields, (int)first);
    int next0 = gu_next0(fields, nfields, fi, tiles);
    for (int tile = (int)first; tile < end; tile += GU_THREADS / 64) {
        while (tile >= next0) next0 = gu_next0(fields, nfields, ++fi, tiles);
        const p4c_grib_field* f = fields + fi;
        const int64_t bitmap_off = f->bitmap_off;
        if (bitmap_off < 0) continue;
        const int N = f->ni * f->nj;
        const int64_t p0 = (int64_t)(tile - f->tile0) * GU_TILE + lane * 32;   // past N - 1 for the lanes behind a short last tile
        const int valid = N - p0 < 32 ? (int)(N - p0) : 32;
        const unsigned char* __restrict__ src = bytes + bitmap_off + (p0 >> 3);   // a multiple of 4: bitmap_off is one
        uint32_t n = 0u;
        if (valid == 32) {
            n = __popc(*reinterpret_cast<const uint32_t*>(src));
        } else {
            for (int j = 0; 8 * j < valid; ++j) n += __popc(gu_presence(src, 8 * j, valid - 8 * j));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (lane == 0) counts[tile] = n;
    }
}

// the 8 points of a lane: point i is present when bit 7 - i of `mask` is set, the first present one has rank k0.  STAGED: the words
// of the stream from word w_lo on lie in `stage`, byte-swapped; otherwise they are loaded from the stream itself.
template <bool STAGED>
__device__ __forceinline__ void gu_decode(float (&out)[8], uint32_t mask, uint32_t k0, const p4c_grib_field& f,
                                          const unsigned char* __restrict__ sp, const uint32_t* stage, int64_t w_lo, double R, double pw) {
    const int nbits = f.nbits;
    int64_t k = k0;
    int64_t bit = k * nbits, wi = -1;
    uint32_t hi = 0u, lo = 0u;
    auto word = [&](int64_t i) { return STAGED ? stage[i - w_lo] : gu_word(sp, i, f.stream_len); };
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        out[i] = NAN;
        if (!((mask >> (7 - i)) & 1u)) continue;
        if (k < f.count) {   // every bit of such a value lies inside ceil(count*nbits/8) <= stream_len bytes
            uint32_t X = 0u;
            if (nbits > 0) {
                const int64_t at = bit >> 5;
                if (wi < 0) {
                    hi = word(at);
                    lo = word(at + 1);
                } else if (at != wi) {   // nbits <= 32: the window moves by one word at most
                    hi = lo;
                    lo = word(at + 1);
                }
                wi = at;
                const uint64_t window = ((uint64_t)hi << 32) | lo;
                X = (uint32_t)((window << (bit & 31)) >> (64 - nbits));
                bit += nbits;
            }
            out[i] = gu_value(X, R, f.E, f.D, pw);
        }
        ++k;
    }
}

// workgroup b takes the tiles [b*per, (b+1)*per) one after the other: the field changes seldom and, with a bitmap, the rank the
// next tile starts at is the one this tile ends at
__global__ void __launch_bounds__(GU_THREADS)
    grib_unpack_kernel(const unsigned char* __restrict__ bytes, const p4c_grib_field* __restrict__ fields, int nfields,
                       float* __restrict__ planes, const uint32_t* __restrict__ counts, int tiles, int per) {
    __shared__ uint32_t wave_s[GU_THREADS / 64], base_s[GU_THREADS / 64];
    __shared__ uint32_t stage_s[GU_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t first = (int64_t)blockIdx.x * per;
    const int end = first + per < tiles ? (int)(first + per) : tiles;
    if (first >= end) return;
    int fi = gu_field_of(fields, nfields, (int)first);
    int next0 = gu_next0(fields, nfields, fi, tiles);
    p4c_grib_field f = fields[fi];
    bool carried = false;      // `rank` is the rank this tile starts at: the previous trip decoded the tile before it
    uint32_t rank = 0u;
    for (int tile = (int)first; tile < end; ++tile) {
        if (tile >= next0) {   // every field has a tile: the next one
            f = fields[++fi];
            next0 = gu_next0(fields, nfields, fi, tiles);
            carried = false;
        }
        const int N = f.ni * f.nj;
        const int t = tile - f.tile0;
        const int64_t p64 = (int64_t)t * GU_TILE + tid * 8;
        const int valid = N - p64 < 8 ? (int)(N - p64) : 8;   // <= 0: the lane is past the field
        const int p0 = (int)p64;                               // used where valid > 0: below 2^31 there
        const bool has_bitmap = f.bitmap_off >= 0;             // the same for the whole workgroup, as all of f
        const unsigned char* __restrict__ sp = bytes + f.stream_off;
        const int nbits = f.nbits;
        uint32_t mask, k0;
        int64_t w_lo = 0;
        if (has_bitmap) {
            mask = gu_presence(bytes + f.bitmap_off, p0, valid);
            const uint32_t n = __popc(mask);
            uint32_t before = 0u;   // the field's earlier tiles
            if (!carried)
                for (int i = tid; i < t; i += GU_THREADS) before += counts[f.tile0 + i];
            uint32_t inc = n;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(inc, o, 64);
                if (lane >= o) inc += v;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
            __syncthreads();   // the previous trip's readers of the slots and of the staged words are done
            if (lane == 63) wave_s[wv] = inc;
            if (lane == 0) base_s[wv] = before;
            __syncthreads();
            const uint32_t base = carried ? rank : base_s[0] + base_s[1] + base_s[2] + base_s[3];
            uint32_t upto = base;
            for (int w = 0; w < wv; ++w) upto += wave_s[w];
            k0 = upto + inc - n;
            rank = base + wave_s[0] + wave_s[1] + wave_s[2] + wave_s[3];
            carried = true;
            // the tile's values are one piece of the stream: bits [base*nbits, last*nbits), staged with coalesced loads
            const int64_t last = rank < (uint32_t)f.count ? rank : f.count;
            int words = 0;
            if (nbits > 0 && (int64_t)base < last) {
                w_lo = ((int64_t)base * nbits) >> 5;
                words = (int)(((last * nbits + 31) >> 5) - w_lo) + 1;   // and the second word of the last value's window
            }
            for (int i = tid; i < words; i += GU_THREADS) stage_s[i] = gu_word(sp, w_lo + i, f.stream_len);
            __syncthreads();
        } else {
            mask = valid >= 8 ? 0xffu : valid > 0 ? (0xff00u >> valid) & 0xffu : 0u;
            k0 = (uint32_t)p0;
        }
        if (valid <= 0) continue;   // after the barriers
        const double R = (double)f.R;
        const double pw = gu_pow10[f.D >= 0 ? f.D : -f.D];
        float out[8];
        if (gu_fast(nbits, has_bitmap) && valid == 8) {
            // count == N here, so the 16 bytes lie inside the stream
            const GuWords4 q = *reinterpret_cast<const GuWords4*>(sp + 2 * (int64_t)p0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t s = __builtin_bswap32(q.w[j]);
                out[2 * j] = gu_value(s >> 16, R, f.E, f.D, pw);
                out[2 * j + 1] = gu_value(s & 0xffffu, R, f.E, f.D, pw);
            }
        } else if (has_bitmap) {
            gu_decode<true>(out, mask, k0, f, sp, stage_s, w_lo, R, pw);
        } else {
            gu_decode<false>(out, mask, k0, f, sp, stage_s, 0, R, pw);
        }
        float* __restrict__ plane = planes + f.dst_off;
        int r = 0, c = 0;
        bool run = valid == 8;   // 8 consecutive plane elements
        int64_t d0 = p0;
        if (f.flip_rows) {
            r = p0 / f.ni;
            c = p0 - r * f.ni;
            run = run && c + 8 <= f.ni;
            d0 = (int64_t)(f.nj - 1 - r) * f.ni + c;
        }
        if (run && (reinterpret_cast<uintptr_t>(plane + d0) & 15) == 0) {   // always, without flip_rows, in a 16-byte aligned `planes`
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
}

}  // namespace p4c

using namespace p4c;

extern "C" int p4c_grib_unpack_tile(void) { return GU_TILE; }
extern "C" int p4c_grib_unpack_max_blocks(void) { return GU_MAX_BLOCKS; }
extern "C" int p4c_grib_unpack_fast(int nbits, int has_bitmap) { return gu_fast(nbits, has_bitmap != 0) ? 1 : 0; }
extern "C" size_t p4c_grib_unpack_workspace_bytes(int64_t tiles) { return tiles > 0 ? (size_t)tiles * sizeof(uint32_t) : 0; }

extern "C" int p4c_grib_unpack(const unsigned char* bytes, int64_t nbytes, const p4c_grib_field* fields,
                               const p4c_grib_field* fields_host, int nfields, float* planes, void* workspace, p4c_stream_t stream) {
    P4C_CHECK_ARG(bytes && fields && fields_host && planes, "p4c_grib_unpack: null pointer");
    P4C_CHECK_ARG((reinterpret_cast<uintptr_t>(bytes) & 3) == 0 && (reinterpret_cast<uintptr_t>(planes) & 3) == 0,
                  "p4c_grib_unpack: bytes and planes must be 4-byte aligned");
    P4C_CHECK_ARG(nfields > 0 && nbytes >= 0, "p4c_grib_unpack: %d fields in %lld bytes", nfields, (long long)nbytes);
    int64_t tiles = 0;
    bool any_bitmap = false;
    for (int i = 0; i < nfields; ++i) {
        const p4c_grib_field& f = fields_host[i];
        P4C_CHECK_ARG(f.ni > 0 && f.nj > 0, "p4c_grib_unpack: field %d: a grid of %d x %d", i, f.nj, f.ni);
        const int64_t N = (int64_t)f.ni * f.nj;
        P4C_CHECK_ARG(N < ((int64_t)1 << 31), "p4c_grib_unpack: field %d: %lld points: at most 2^31 - 1", i, (long long)N);
        P4C_CHECK_ARG(f.nbits >= 0 && f.nbits <= 32 && f.D >= -GU_MAX_D && f.D <= GU_MAX_D,
                      "p4c_grib_unpack: field %d: nbits = %d, D = %d (0 <= nbits <= 32 and |D| <= %d)", i, f.nbits, f.D, GU_MAX_D);
        P4C_CHECK_ARG(f.count >= 0 && f.count <= N, "p4c_grib_unpack: field %d: %d values for %lld points", i, f.count, (long long)N);
        P4C_CHECK_ARG(f.bitmap_off >= -1, "p4c_grib_unpack: field %d: bitmap_off = %lld (-1: no bitmap)", i, (long long)f.bitmap_off);
        P4C_CHECK_ARG(f.bitmap_off >= 0 || f.count == N, "p4c_grib_unpack: field %d: no bitmap and %d values for %lld points", i, f.count,
                      (long long)N);
        P4C_CHECK_ARG(f.stream_off >= 0 && (f.stream_off & 3) == 0 && (f.bitmap_off < 0 || (f.bitmap_off & 3) == 0) && f.dst_off >= 0 &&
                          (f.dst_off & 3) == 0,
                      "p4c_grib_unpack: field %d: stream_off = %lld, bitmap_off = %lld, dst_off = %lld: multiples of 4, not negative", i,
                      (long long)f.stream_off, (long long)f.bitmap_off, (long long)f.dst_off);
        const int64_t need = ((int64_t)f.count * f.nbits + 7) / 8;
        P4C_CHECK_ARG(f.stream_len >= need, "p4c_grib_unpack: field %d: a stream of %lld bytes for %d values of %d bits", i,
                      (long long)f.stream_len, f.count, f.nbits);
        P4C_CHECK_ARG(f.stream_off <= nbytes && f.stream_len <= nbytes - f.stream_off,
                      "p4c_grib_unpack: field %d: the stream [%lld, +%lld) leaves the %lld bytes", i, (long long)f.stream_off,
                      (long long)f.stream_len, (long long)nbytes);
        P4C_CHECK_ARG(f.bitmap_off < 0 || (f.bitmap_off <= nbytes && (N + 7) / 8 <= nbytes - f.bitmap_off),
                      "p4c_grib_unpack: field %d: the bitmap [%lld, +%lld) leaves the %lld bytes", i, (long long)f.bitmap_off,
                      (long long)((N + 7) / 8), (long long)nbytes);
        P4C_CHECK_ARG(f.tile0 == tiles, "p4c_grib_unpack: field %d: tile0 = %d, the tiles before it are %lld", i, f.tile0, (long long)tiles);
        tiles += (N + GU_TILE - 1) / GU_TILE;
        P4C_CHECK_ARG(tiles < ((int64_t)1 << 31), "p4c_grib_unpack: %lld tiles: at most 2^31 - 1 per call", (long long)tiles);
        any_bitmap = any_bitmap || f.bitmap_off >= 0;
    }
    P4C_CHECK_ARG(!any_bitmap || workspace, "p4c_grib_unpack: null workspace for fields with a bitmap");
    const int per = (int)((tiles + GU_MAX_BLOCKS - 1) / GU_MAX_BLOCKS);   // consecutive tiles of a workgroup
    const unsigned blocks = (unsigned)((tiles + per - 1) / per);
    hipStream_t st = as_stream(stream);
    uint32_t* counts = (uint32_t*)workspace;
    if (any_bitmap) {
        hipLaunchKernelGGL(grib_count_kernel, dim3(blocks), dim3(GU_THREADS), 0, st, bytes, fields, nfields, counts, (int)tiles, per);
        P4C_CHECK_LAUNCH("p4c_grib_unpack(count)");
    }
    hipLaunchKernelGGL(grib_unpack_kernel, dim3(blocks), dim3(GU_THREADS), 0, st, bytes, fields, nfields, planes, (const uint32_t*)counts,
                       (int)tiles, per);
    P4C_CHECK_LAUNCH("p4c_grib_unpack(unpack)");
    return P4C_OK;
}
