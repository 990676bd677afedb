// conv3x3_bf16_small: 3x3 convolution 64 -> 64 channels on bf16 NHWC maps that are small enough for a launch to be pure latency
// (the coarse levels of the HalfUNet plan: B x H x W up to about one tile per CU).  Built for latency, not throughput -- the
// row-streaming kernel (conv_rows.hip) pays a six-row pipeline fill / drain, a 144-register weight prologue in front of its first
// interval and four statistics slots per workgroup for two rows of output there:
//
//   * ONE tile per workgroup, one pass: TR output rows x 32 columns x 64 output channels of one sample; no role split, no row ring,
//     no persistent loop.  TR (2 / 4 / 8 / 16) is chosen on the host so that the launch has at most one workgroup per CU;
//   * 256 threads.  Every lane issues ALL its loads at once: its slots of the (TR + 2) x 34 halo tile (16-byte buffer loads,
//     out-of-range offsets give the zero padding), then the 36 A operands of its wave (the row kernel's prepared image, unchanged);
//   * the halo tile is transformed on the way in (plain, or relu(y * scale + shift): xform2<2>) and written to LDS in the row
//     kernel's 144-byte padded pixels -- every B operand is `row base + immediate`, conflict-free; ONE barrier;
//   * wave = (output-channel half, every other row of the tile): 36 MFMAs per output row from a zero accumulator in the row kernel's
//     order (tap row 0, 1, 2; column shift 0, 1, 2; channel slice 0 .. 3), so the stored map is bit-identical to its;
//   * accumulators -> bf16 -> LDS staging (the row kernel's swizzle) -> barrier -> 16-byte coalesced stores by all 256 lanes, which
//     also take the channel sums of the stored (rounded) values: ONE slot [2][64] per workgroup, combined over the four waves in a
//     fixed order.  BatchNorm is finished in place by the last workgroup (BatchFin, as in the row kernel).
//   * where the level's SECOND convolution is this kernel too, the first one leaves its slots and ends, and the second finishes them
//     in its prologue (PRE below): no ticket and no last-workgroup tail between the two launches;
// LDS at TR = 16: halo tile 18 x 34 x 144 B = 86.1 KB + staging 16 x 32 x 128 B = 64 KB = 150.1 KB (one workgroup per CU).
#include <stddef.h>
#include <stdlib.h>

#include "kernels.hpp"

namespace p4c {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

namespace sm {
constexpr int TW = 32;                 // tile width (output pixels)
constexpr int LW = TW + 2;             // input columns of a tile
constexpr int PIXB = 144;              // LDS bytes of an input pixel: 64 bf16 channels + 16 B pad (conv_rows.hip: Lay<32>)
constexpr int RROW = LW * PIXB;        // one input row
constexpr int ROWSLOTS = LW * 8;       // 16-byte slots per input row
constexpr int SROW = TW * 128;         // one staged output row
constexpr int TR_MAX = 16;
template <int TR> struct Geo {
    static constexpr int NSLOT = (TR + 2) * ROWSLOTS;
    static constexpr int NLD = (NSLOT + 255) / 256;     // input slots per lane
    static constexpr int INB = (TR + 2) * RROW;
    static constexpr int SMEM = INB + TR * SROW;
};
static_assert(Geo<TR_MAX>::SMEM <= 160 * 1024, "LDS of the largest tile");
// the statistics tail reuses the (dead) halo tile: [4 waves][128] floats, [8][128] doubles, one flag
static_assert(Geo<2>::INB >= 4 * 128 * 4 + 8 * 128 * 8 + 16, "reduction scratch fits the smallest halo tile");
}  // namespace sm

constexpr int OOB = 0x7fffffff;

// relu(v * scale + shift) on the 2 bf16 channels packed in one word: conv_rows.hip's xform2<2>, as it stands
__device__ __forceinline__ unsigned int xform_relu2(unsigned int w, f32x2 sc, f32x2 sh) {
    const float lo = __builtin_fmaf(__builtin_bit_cast(float, w << 16), sc.x, sh.x);
    const float hi = __builtin_fmaf(__builtin_bit_cast(float, w & 0xffff0000u), sc.y, sh.y);
    const f32x2 v = {lo, hi};
    w = __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf16x2));
    const s16x2 z = {0, 0};   // negative floats are negative int16: max(., 0) clears them
    return __builtin_bit_cast(unsigned int, __builtin_elementwise_max(__builtin_bit_cast(s16x2, w), z));
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

// workgroup barrier that orders LDS traffic only: global loads / stores stay in flight across it
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

struct SmallArgs {
    const __bf16* in; const __bf16* wp; const float* in_scale; const float* in_shift; __bf16* out; float* stat_partial;
    int H, W, fin_on;
    BatchFin fin;   // this launch's statistics, finished by its last workgroup
    BatchFin pre;   // PRE: the PRODUCER's statistics (slots it left, one per workgroup of the same grid), finished in this launch's prologue
};
// a field of the argument struct loaded at the point of use (conv_rows.hip: late_arg): the finalize's pointers are not held in
// scalar registers through the kernel
template <typename T>
__device__ __forceinline__ T late_arg(size_t offset) {
#if defined(__HIP_DEVICE_COMPILE__)
    const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *reinterpret_cast<const T*>(ka + offset);
#else
    (void)offset;
    return T{};
#endif
}

// Combine of `n` statistics slots [2][64] by one workgroup of 256 threads, as BatchFin's last workgroup does it (conv_rows.hip): thread =
// (column quad cq, slot group sg) sums the slots sg, sg + 8, sg + 16, ... in increasing order in fp64; the eight groups are then added
// in order by finish_channel().  Up to 32 loads in flight per thread (the additions keep their order).
__device__ __forceinline__ void combine_slots(const float* slots, int n, int tid, double* dred) {
    const int cq = tid & 31, sg = tid >> 5;
    double acc4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s0 = sg; s0 < n; s0 += 8 * 32) {   // (one trip up to 256 slots: every load of the thread in flight at once)
        p4c_f32x4 v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            const int sl = s0 + 8 * u;
            v[u] = sl < n ? *(reinterpret_cast<const p4c_f32x4*>(slots + (int64_t)sl * 128) + cq) : p4c_f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 32; ++u) { acc4[0] += v[u].x; acc4[1] += v[u].y; acc4[2] += v[u].z; acc4[3] += v[u].w; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) dred[sg * 128 + 4 * cq + k] = acc4[k];
}

// Channel c from the eight group sums: scale / shift / mean / rstd, the arithmetic of norm_finalize (norm_pool.hip) operation by
// operation -- contraction is spelled out, so the in-kernel finish, the consumer-side finish and that launch give the same bits.
// publish: write the (B,64) arrays and update the running statistics (torch semantics: the biased variance normalises, the unbiased
// one is tracked).
struct ChanNorm { float scale, shift; };
__device__ __forceinline__ ChanNorm finish_channel(const BatchFin& fin, const double* dred, int c, bool publish) {
#pragma clang fp contract(off)
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int g8 = 0; g8 < 8; ++g8) { s1 += dred[g8 * 128 + c]; s2 += dred[g8 * 128 + 64 + c]; }
    const double n = fin.count;
    const double mean = s1 / n;
    double var = __builtin_fma(-mean, mean, s2 / n);
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + (double)fin.eps));
    const float scl = fin.gamma[c] * rstd, shf = __builtin_fmaf(-(float)mean, scl, fin.beta[c]);
    if (publish) {
        if (fin.running_mean) {
            const double unbiased = n > 1.0 ? var * n / (n - 1.0) : var;
            const float keep = 1.f - fin.momentum;
            const float m0 = keep * fin.running_mean[c], m1 = fin.momentum * (float)mean;
            const float v0 = keep * fin.running_var[c], v1 = fin.momentum * (float)unbiased;
            fin.running_mean[c] = m0 + m1;
            fin.running_var[c] = v0 + v1;
        }
        for (int bb = 0; bb < fin.B; ++bb) {
            fin.scale[bb * 64 + c] = scl; fin.shift[bb * 64 + c] = shf; fin.mean[bb * 64 + c] = (float)mean; fin.rstd[bb * 64 + c] = rstd;
        }
    }
    return ChanNorm{scl, shf};
}

// MODE 0: plain input (a pooled map), 2: relu(y * scale + shift) of the producing normalisation.
// PRE (MODE 2): the producer -- the level's first convolution, a launch of this kernel on the same grid -- left its statistics slots
// and ended (no ticket, no tail); every workgroup of this launch reads them beside its weights and combines them as BatchFin would
// (same order: every workgroup gets the same bits), and workgroup 0 publishes scale / shift / mean / rstd and the running statistics
// for the backward's consumers.
template <int MODE, int TR, bool PRE>
__global__ void __launch_bounds__(256) conv3x3_bf16_small_kernel(SmallArgs args) {
    static_assert(!PRE || MODE == 2, "the consumer-side finish feeds the input transform");
    using namespace sm;
    typedef Geo<TR> G;
    constexpr int NLD = G::NLD;
    const __bf16* __restrict__ in = args.in;
    const __bf16* __restrict__ wp = args.wp;
    __bf16* __restrict__ out = args.out;
    const int H = args.H, W = args.W;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* lin = smem;
    char* lstg = smem + G::INB;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = lane & 31, h = lane >> 5, c8 = tid & 7;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TR, b = blockIdx.z;
    const int wg_id = (b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, wg_count = gridDim.x * gridDim.y * gridDim.z;
    const int ct = wv & 1, rg = wv >> 1;   // wave: output channels 32 ct .. +31, tile rows rg, rg + 2, ...

    // ---- every load of the workgroup, at once: the lane's slots of the halo tile, then the wave's weights
    const __amdgpu_buffer_rsrc_t rs_in = make_rsrc(in + (int64_t)b * H * W * 64, (unsigned int)H * W * 128u);
    u32x4 img[NLD];
    unsigned int inside = 0;   // bit `it`: the slot is a pixel of the image
#pragma unroll
    for (int it = 0; it < NLD; ++it) {
        const int idx = tid + it * 256, row = idx / ROWSLOTS, col = (idx - row * ROWSLOTS) >> 3;   // (256 and ROWSLOTS are multiples of 8: the octet is c8)
        const int gy = y0 - 1 + row, gx = x0 - 1 + col;
        const bool ok = (idx < G::NSLOT) & ((unsigned)gy < (unsigned)H) & ((unsigned)gx < (unsigned)W);
        inside |= ok ? 1u << it : 0u;
        img[it] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, ok ? (gy * W + gx) * 128 + 16 * c8 : OOB, 0, 0);
    }
    f32x2 sc[4], sh[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sc[k] = sh[k] = f32x2{0.f, 0.f};
        if (MODE == 2 && !PRE) {
            sc[k] = *reinterpret_cast<const f32x2*>(args.in_scale + b * 64 + 8 * c8 + 2 * k);
            sh[k] = *reinterpret_cast<const f32x2*>(args.in_shift + b * 64 + 8 * c8 + 2 * k);
        }
    }
    bf16x8 A[9][4];
    {
        const char* wsrc = reinterpret_cast<const char*>(wp) + (h * 64 + ct * 32 + r) * 16;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) A[tap][ks] = *reinterpret_cast<const bf16x8*>(wsrc + (tap * 4 + ks) * 2048);
    }
    if (PRE) {
        // the producer's statistics (BatchNorm: one scale / shift per channel for every sample).  Group sums in the halo tile's LDS
        // (not yet written), the 64 channels' scale / shift in the staging area (not written before the matrix phase).
        const BatchFin pre = late_arg<BatchFin>(offsetof(SmallArgs, pre));
        double* dred = reinterpret_cast<double*>(lin);
        float* lnorm = reinterpret_cast<float*>(lstg);   // [2][64]
        combine_slots(pre.slots, wg_count, tid, dred);
        lds_barrier();
        if (tid < 64) {
            const ChanNorm cn = finish_channel(pre, dred, tid, wg_id == 0);
            lnorm[tid] = cn.scale;
            lnorm[64 + tid] = cn.shift;
        }
        lds_barrier();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sc[k] = *reinterpret_cast<const f32x2*>(lnorm + 8 * c8 + 2 * k);
            sh[k] = *reinterpret_cast<const f32x2*>(lnorm + 64 + 8 * c8 + 2 * k);
        }
    }

    // ---- halo tile -> LDS (zero padding applies to the NORMALISED activation: out-of-image slots are cleared after the transform)
#pragma unroll
    for (int it = 0; it < NLD; ++it) {
        const int idx = tid + it * 256, row = idx / ROWSLOTS, col = (idx - row * ROWSLOTS) >> 3;
        u32x4 o = img[it];
        if (MODE == 2) {
            const unsigned int keep = (inside >> it) & 1u ? 0xffffffffu : 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = xform_relu2(o[k], sc[k], sh[k]) & keep;
        }
        if (idx < G::NSLOT) *reinterpret_cast<u32x4*>(lin + row * RROW + col * PIXB + 16 * c8) = o;
    }
    lds_barrier();

    // ---- matrix phase: output row `row` of the tile = 36 MFMAs on input rows row .. row + 2 (C[co][px]: lane = pixel column r (+ half
    // h), register quad g -> channels 32 ct + 8 g + 4 h .. + 3)
    {
        const int lane_base = r * PIXB + 16 * h;   // B operand (ky, kx, ks) of output row j: + (j + ky) * RROW + kx * PIXB + 32 * ks
        int soff[4];                               // staging offsets of the lane's 4 channel quads (slot XOR (px >> 1) & 7)
#pragma unroll
        for (int g = 0; g < 4; ++g) soff[g] = r * 128 + 8 * h + (((4 * ct + g) ^ ((r >> 1) & 7)) << 4);
#pragma unroll 1
        for (int row = rg; row < TR; row += 2) {
            if (y0 + row >= H) break;
            const char* rb = lin + row * RROW + lane_base;
            auto bop = [&](int t) __attribute__((always_inline)) {
                const int ky = t / 12, q = t % 12;
                return *reinterpret_cast<const bf16x8*>(rb + ky * RROW + (q >> 2) * PIXB + (q & 3) * 32);
            };
            bf16x8 fb[8];
#pragma unroll
            for (int t = 0; t < 6; ++t) fb[t] = bop(t);
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
            for (int t = 0; t < 36; ++t) {
                if (t + 6 < 36) fb[(t + 6) & 7] = bop(t + 6);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[t >> 2][t & 3], fb[t & 7], acc, 0, 0, 0);
            }
            char* stg = lstg + row * SROW;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x2 lo = {acc[4 * g], acc[4 * g + 1]}, hi = {acc[4 * g + 2], acc[4 * g + 3]};
                u32x2 o;
                o[0] = __builtin_bit_cast(unsigned int, __builtin_convertvector(lo, bf16x2));
                o[1] = __builtin_bit_cast(unsigned int, __builtin_convertvector(hi, bf16x2));
                *reinterpret_cast<u32x2*>(stg + soff[g]) = o;
            }
        }
    }
    lds_barrier();   // every row is staged; the halo tile is dead from here on

    // ---- drain: lane = (pixel column tid >> 3, channel octet c8) of every tile row
    const __amdgpu_buffer_rsrc_t rs_out = make_rsrc(out + (int64_t)b * H * W * 64, (unsigned int)H * W * 128u);
    const int col = tid >> 3, gx = x0 + col;
    u32x4 v[TR];
    float a1[8], a2[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) a1[q] = a2[q] = 0.f;
    {
        const int sofs = col * 128 + ((c8 ^ ((col >> 1) & 7)) << 4);
#pragma unroll
        for (int j = 0; j < TR; ++j) {
            v[j] = *reinterpret_cast<const u32x4*>(lstg + j * SROW + sofs);
            if (!((y0 + j < H) & (gx < W))) v[j] = u32x4{0u, 0u, 0u, 0u};   // (rows beyond the image were never staged) keeps the statistics unmasked
            if (args.stat_partial) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float lo = __builtin_bit_cast(float, v[j][q] << 16);
                    const float hi = __builtin_bit_cast(float, v[j][q] & 0xffff0000u);
                    a1[2 * q] += lo; a2[2 * q] = __builtin_fmaf(lo, lo, a2[2 * q]);
                    a1[2 * q + 1] += hi; a2[2 * q + 1] = __builtin_fmaf(hi, hi, a2[2 * q + 1]);
                }
            }
        }
    }
    auto store_rows = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < TR; ++j) {
            const bool valid = (y0 + j < H) & (gx < W);
            __builtin_amdgcn_raw_buffer_store_b128(v[j], rs_out, valid ? ((y0 + j) * W + gx) * 128 + 16 * c8 : OOB, 0, 0);
        }
    };
    if (!args.stat_partial || !args.fin_on) store_rows();
    if (!args.stat_partial) return;

    // ---- channel statistics: lanes of one octet within a wave, then the four waves in a fixed order: ONE slot per workgroup
    float* lred = reinterpret_cast<float*>(lin);                       // [4 waves][128], then doubles [8][128]
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        float u = a1[q], w2 = a2[q];
        u += __shfl_xor(u, 8); w2 += __shfl_xor(w2, 8);
        u += __shfl_xor(u, 16); w2 += __shfl_xor(w2, 16);
        u += __shfl_xor(u, 32); w2 += __shfl_xor(w2, 32);
        if (lane < 8) { lred[wv * 128 + 8 * c8 + q] = u; lred[wv * 128 + 64 + 8 * c8 + q] = w2; }
    }
    lds_barrier();
    if (!args.fin_on) {
        if (tid < 128) args.stat_partial[(int64_t)wg_id * 128 + tid] = (lred[tid] + lred[128 + tid]) + (lred[256 + tid] + lred[384 + tid]);
        return;
    }
    // ---- BatchNorm finished in place (kernels.hpp: BatchFin; the row kernel's tail): slot, ticket, the last workgroup combines.  The
    // slot and the ticket go out BEFORE the output rows: the wait for the slot's acknowledgement then covers 128 floats, not the tile.
    const BatchFin fin = late_arg<BatchFin>(offsetof(SmallArgs, fin));
    unsigned int* lflag = reinterpret_cast<unsigned int*>(lred + 4 * 128 + 8 * 256);
    if (wv == 0) {
        // device-scope (write-through) stores, then the ticket once they are acknowledged: no release fence
#pragma unroll
        for (int j = lane; j < 128; j += 64)
            __hip_atomic_store(fin.slots + (int64_t)wg_id * 128 + j, (lred[j] + lred[128 + j]) + (lred[256 + j] + lred[384 + j]),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) *lflag = __hip_atomic_fetch_add(fin.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    store_rows();
    lds_barrier();
    if (*lflag != (unsigned)wg_count - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // invalidate only: the other workgroups' slots are read from memory
    double* dred = reinterpret_cast<double*>(lred + 4 * 128);   // [8][128]
    combine_slots(fin.slots, wg_count, tid, dred);
    lds_barrier();
    if (tid < 64) finish_channel(fin, dred, tid, true);
    if (tid == 0) __hip_atomic_store(fin.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Tile rows of a launch: the smallest of 2 / 4 / 8 / 16 that leaves at most one workgroup per CU (more rows per tile = fewer halo
// rows re-read, but every wave then walks more rows one after the other); 0: the map is too large for one round of workgroups.
int small_tile_rows(int B, int H, int W) {
    const int ntx = (W + sm::TW - 1) / sm::TW, cus = num_cus();
    for (int tr = 2; tr <= sm::TR_MAX; tr *= 2)
        if ((int64_t)B * ((H + tr - 1) / tr) * ntx <= cus) return tr;
    return 0;
}

bool small_shape_ok(int storage, int B, int H, int W) {   // what the kernel can run at all (any width, any height)
    return storage == P4C_BF16 && B > 0 && H > 0 && W > 0 && B <= 65535 && (int64_t)H * W * 128 < (int64_t)1 << 31;
}

template <int MODE, int TR, bool PRE>
int launch_small(const SmallArgs& args, int B, int H, int W, hipStream_t stream) {
    typedef sm::Geo<TR> G;
    P4C_TRY(ensure_dyn_smem((const void*)conv3x3_bf16_small_kernel<MODE, TR, PRE>, G::SMEM));
    hipLaunchKernelGGL((conv3x3_bf16_small_kernel<MODE, TR, PRE>), dim3((W + sm::TW - 1) / sm::TW, (H + TR - 1) / TR, B), dim3(256),
                       G::SMEM, stream, args);
    return P4C_OK;
}

template <int MODE, bool PRE>
int launch_small_tr(const SmallArgs& args, int tr, int B, int H, int W, hipStream_t stream) {
    switch (tr) {
        case 2: return launch_small<MODE, 2, PRE>(args, B, H, W, stream);
        case 4: return launch_small<MODE, 4, PRE>(args, B, H, W, stream);
        case 8: return launch_small<MODE, 8, PRE>(args, B, H, W, stream);
        default: return launch_small<MODE, 16, PRE>(args, B, H, W, stream);
    }
}

}  // namespace

// Routing threshold (HalfUNet plan, conv_block_fwd): the shapes at which the interleaved micro-benchmark showed this kernel faster
// than the row / ring kernel in all three forward modes (profiles/small_conv_micro.txt).  P4C_SMALL_CONV=0 (diagnostic library):
// the earlier routing; P4C_SMALL_CONV_MAX_PIXELS overrides the threshold there.
bool conv_small_ok(int storage, int B, int H, int W) {
    const char* e = diag_env("P4C_SMALL_CONV");   // (read per call: the A/B scripts and the parity tests switch it)
    if (e && e[0] == '0') return false;
    int64_t max_pixels = (int64_t)2 * 128 * 160;   // (2 x 256 x 256: the row kernel is 1.5 us faster in every mode)
    if (const char* m = diag_env("P4C_SMALL_CONV_MAX_PIXELS")) max_pixels = atoll(m);
    return small_shape_ok(storage, B, H, W) && small_tile_rows(B, H, W) > 0 && (int64_t)B * H * W <= max_pixels;
}

int conv_small_stat_slots(int B, int H, int W) {
    int tr = small_tile_rows(B, H, W);
    if (tr == 0) tr = sm::TR_MAX;
    return ((H + tr - 1) / tr) * ((W + sm::TW - 1) / sm::TW);
}

// the consumer-side finish: the producer's slots are one per workgroup of the SAME grid, few enough for every workgroup to combine
bool conv_small_handoff_ok(int storage, int B, int H, int W) {
    const char* e = diag_env("P4C_SMALL_HANDOFF");   // (A/B switch and parity tests)
    if (e && e[0] == '0') return false;
    return conv_small_ok(storage, B, H, W) && B * conv_small_stat_slots(B, H, W) <= 256;
}

int launch_conv3x3_bf16_small(const void* in, const void* wp, const float* in_scale, const float* in_shift, int in_relu, void* out,
                              float* stat_partial, int B, int H, int W, hipStream_t stream, const BatchFin* finp, const BatchFin* prep) {
    if (!small_shape_ok(P4C_BF16, B, H, W)) return fail(P4C_ERR_UNSUPPORTED, "conv_bf16_small: unsupported shape (%dx%dx%d)", B, H, W);
    P4C_CHECK_ARG((in_scale != nullptr) == (in_shift != nullptr) && ((in_scale != nullptr) || prep != nullptr) == (in_relu != 0) &&
                      !(in_scale && prep),
                  "conv_bf16_small: the input is plain or relu(y * scale + shift), scale / shift given or finished from the producer's slots");
    P4C_CHECK_ARG(!finp || stat_partial, "conv_bf16_small: the in-kernel finalize needs the slot buffer");
    P4C_CHECK_ARG(!prep || (prep->slots && prep->slots != stat_partial && B * conv_small_stat_slots(B, H, W) <= 256),
                  "conv_bf16_small: the consumer-side finish needs the producer's slots (at most 256, in a buffer of their own)");
    int tr = small_tile_rows(B, H, W);
    if (tr == 0) tr = sm::TR_MAX;   // (more than one round of workgroups: correct, and never routed -- the micro-benchmark's large shapes)
    SmallArgs args{(const __bf16*)in, (const __bf16*)wp, in_scale, in_shift, (__bf16*)out, stat_partial, H, W, finp ? 1 : 0, BatchFin{}, BatchFin{}};
    if (finp) { args.fin = *finp; args.fin.slots = stat_partial; }
    if (prep) args.pre = *prep;
    prof_begin(P4C_PROF_CONV3X3_C64, (int64_t)B * H * W, stream);
    const int rc = prep ? launch_small_tr<2, true>(args, tr, B, H, W, stream)
                        : in_scale ? launch_small_tr<2, false>(args, tr, B, H, W, stream) : launch_small_tr<0, false>(args, tr, B, H, W, stream);
    prof_end(P4C_PROF_CONV3X3_C64, stream);
    if (rc != P4C_OK) return rc;
    P4C_CHECK_LAUNCH("conv_bf16_small");
    return P4C_OK;
}

}  // namespace p4c
