// Evaluation sums: what the score-card and spatial-error observers of a validation / test step need, in ONE streaming pass over
// prediction and target (py4cast/plots.py:488-651 call ScaledLoss twice and WeightedLoss(reduce_spatial_dim=False) once, plus the
// union-mask count of losses.py:197 -- three to four passes, each followed by a collective and a blocking host copy).
//
//   scores[0,b,t,f] = std[f] *      sum_n interior[n] |d| / (num_interior - masked_count)          d = pred*m - target*m
//   scores[1,b,t,f] = std[f] * sqrt(sum_n interior[n] d*d / (num_interior - masked_count))
//   masked_count    = #{n : m[b,t,n,f] == 0 for every (b,t,f)}
//   map_acc[t,n]  (+)= sum_b sum_f weights[f] * (d*d or |d|)                                        b ascending
//
// The union mask and the sum over b are per grid point, so a workgroup OWNS a range of grid points and walks every (b,t) slab of
// that range (t outer, b inner: the map row of one t is complete after B slabs and is written once).  Per-feature sums leave as
// block partials in the caller's workspace and a small finish launch adds them in a fixed order: no float atomics, two calls on the
// same inputs give the same bits.  HBM-bound: prediction, target and an explicit mask are read once.
//
// Compiled with -ffp-contract=off like losses.hip (the element expression is losses.hip::loss_elem's, rounding for rounding).
#include "common.hpp"

namespace p4c {

constexpr int EV_TILE = 64;             // grid points per tile (<= 64 * 64 elements: 16 KiB of differences in LDS)
constexpr int EV_MAX_TILES = 8;         // tiles per workgroup
constexpr int EV_MAX_R = EV_TILE * EV_MAX_TILES;
constexpr int EV_TARGET_BLOCKS = 1024;  // ~4 workgroups per CU; more only where a workgroup already owns EV_MAX_R points
constexpr int EV_MAX_ITERS = 4;         // scalar path: F <= 256
constexpr int EV_FINAL_THREADS = 1024;

struct EvalGeom {
    int R;         // grid points per workgroup, a multiple of EV_TILE
    int64_t nblk;
};
static inline EvalGeom eval_geom(int64_t N) {
    int64_t tiles = (N + (int64_t)EV_TILE * EV_TARGET_BLOCKS - 1) / ((int64_t)EV_TILE * EV_TARGET_BLOCKS);
    if (tiles < 1) tiles = 1;
    if (tiles > EV_MAX_TILES) tiles = EV_MAX_TILES;
    EvalGeom g;
    g.R = (int)tiles * EV_TILE;
    g.nblk = (N + g.R - 1) / g.R;
    return g;
}

static inline int pow2_ge(int v, int cap) {
    int p = 1;
    while (p < v && p < cap) p <<= 1;
    return p;
}

struct EvalArgs {
    const float* pred;
    int64_t pred_bs, pred_ts;
    const float* target;
    int64_t tgt_bs, tgt_ts;
    const void* mask;   // dense (B,T,N,F) for P4C_MASK_F32 / P4C_MASK_U8
    int mask_mode;
    const float* interior;
    const float* weights;
    int map_kind;       // P4C_LOSS_MSE / P4C_LOSS_L1, or P4C_EVAL_MAP_NONE
    float* map_acc;
    int accumulate;
    float* partial;            // [2][B*T][nblk][F]
    int32_t* count_partial;    // [nblk]
    int B, T;
    int64_t N;
    int F, R;
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// #points of the workgroup's range that no (b,t,f) unmasked -> count_partial[blk]; every thread calls it
__device__ __forceinline__ void eval_store_count(const int* any_s, int n_cnt, int mask_mode, int32_t* count_partial, int* cred) {
    int local = 0;
    if (mask_mode != P4C_MASK_NONE)
        for (int i = threadIdx.x; i < n_cnt; i += 256) local += any_s[i] == 0 ? 1 : 0;
    local = wave_sum_i(local);
    if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) count_partial[blockIdx.x] = (cred[0] + cred[1]) + (cred[2] + cred[3]);
}

// ------------------------------------------------------------------ flat 16-byte path
// N*F % 4 == 0, 16-byte aligned bases and strides, F <= 64.  The (np,F) block of a tile is streamed flat with 16-byte loads -- a
// lane's four elements may straddle grid points, as in the flat AR-step kernels of losses.hip -- and the differences d go through
// an LDS tile: a column walk gives the per-feature sums (lanes over consecutive f: conflict free), a row walk the per-point sums.
// MM: the mask mode, a template argument so that the modes without a mask tensor hold no mask registers
template <int MM>
__global__ void __launch_bounds__(256) eval_sums_flat_kernel(EvalArgs a, unsigned rcp, int FP) {
    __shared__ __attribute__((aligned(16))) float tile[EV_TILE * 64];
    __shared__ float im_s[EV_MAX_R], map_s[EV_MAX_R], w_s[64];
    __shared__ int any_s[EV_MAX_R];
    __shared__ float mq[4][EV_TILE];
    __shared__ float fred[2][256];
    __shared__ int cred[4];
    const int tid = threadIdx.x, F = a.F, R = a.R;
    const int64_t nblk = gridDim.x, nbt = (int64_t)a.B * a.T;
    const int64_t n_begin = (int64_t)blockIdx.x * R;
    const int n_cnt = (int)((a.N - n_begin) < R ? (a.N - n_begin) : R);
    const bool want_map = a.map_acc != nullptr && a.map_kind != P4C_EVAL_MAP_NONE;
    for (int i = tid; i < R; i += 256) {
        im_s[i] = i < n_cnt ? a.interior[n_begin + i] : 0.0f;
        any_s[i] = 0;
    }
    if (tid < 64) w_s[tid] = (want_map && tid < F) ? a.weights[tid] : 0.0f;
    // column walk: thread = (feature fc, chunk ch of the tile's points)
    const int fc = tid & (FP - 1), ch = tid / FP, nch = 256 / FP;
    // row walk: thread = (point mp, quarter mqi of the features); the start is rotated by the point so that the lanes of a wave do
    // not meet on a bank when F is even
    const int mp = tid & 63, mqi = tid >> 6;
    const int f_lo = (F * mqi) / 4, f_len = (F * (mqi + 1)) / 4 - f_lo;
    const int rot = f_len > 0 ? mp % f_len : 0;
    __syncthreads();
    for (int t = 0; t < a.T; ++t) {
        for (int i = tid; i < R; i += 256) map_s[i] = 0.0f;   // (first touched again two barriers later)
        for (int b = 0; b < a.B; ++b) {
            const float* p = a.pred + (int64_t)b * a.pred_bs + (int64_t)t * a.pred_ts + n_begin * F;
            const float* g = a.target + (int64_t)b * a.tgt_bs + (int64_t)t * a.tgt_ts + n_begin * F;
            const int64_t mbase = ((int64_t)b * a.T + t) * a.N * F + n_begin * F;
            float fa1 = 0.0f, fa2 = 0.0f;
            for (int p0 = 0; p0 < n_cnt; p0 += EV_TILE) {
                const int np = (n_cnt - p0) < EV_TILE ? (n_cnt - p0) : EV_TILE;
                const int nvec = (np * F) >> 2;   // p0*F and np*F are multiples of 4 (EV_TILE is, N*F is)
                const int eoff = p0 * F;
                p4c_f32x4 pv[4], gv[4], mv[(MM == P4C_MASK_F32 || MM == P4C_MASK_U8) ? 4 : 1];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int v = tid + 256 * i;
                    pv[i] = gv[i] = p4c_f32x4{0.f, 0.f, 0.f, 0.f};
                    if constexpr (MM == P4C_MASK_F32 || MM == P4C_MASK_U8) mv[i] = p4c_f32x4{1.f, 1.f, 1.f, 1.f};
                    if (v < nvec) {
                        pv[i] = *reinterpret_cast<const p4c_f32x4*>(p + eoff + 4 * v);
                        gv[i] = *reinterpret_cast<const p4c_f32x4*>(g + eoff + 4 * v);
                        if constexpr (MM == P4C_MASK_F32) {
                            mv[i] = *reinterpret_cast<const p4c_f32x4*>((const float*)a.mask + mbase + eoff + 4 * v);
                        } else if constexpr (MM == P4C_MASK_U8) {
                            const uchar4 u = *reinterpret_cast<const uchar4*>((const unsigned char*)a.mask + mbase + eoff + 4 * v);
                            mv[i] = p4c_f32x4{u.x ? 1.f : 0.f, u.y ? 1.f : 0.f, u.z ? 1.f : 0.f, u.w ? 1.f : 0.f};
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int v = tid + 256 * i;
                    if (v < nvec) {
                        int pl = (int)(((unsigned)(4 * v) * rcp) >> 20);   // exact for 4v < 4096, F <= 64 (losses.hip::flat_pf)
                        int f = 4 * v - pl * F;
                        p4c_f32x4 dv;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float tg = gv[i][j], m = 1.0f;
                            if constexpr (MM == P4C_MASK_F32 || MM == P4C_MASK_U8) m = mv[i][j];
                            if (MM == P4C_MASK_FROM_NAN) {
                                const bool isn = tg != tg;
                                m = isn ? 0.0f : 1.0f;
                                if (isn) tg = 0.0f;
                            }
                            const float pm = pv[i][j] * m, tm = tg * m;   // losses.py:144 / 195
                            dv[j] = pm - tm;
                            if (MM != P4C_MASK_NONE && m != 0.0f) any_s[p0 + pl] = 1;   // (same value from every writer)
                            if (++f == F) {
                                f = 0;
                                ++pl;
                            }
                        }
                        *reinterpret_cast<p4c_f32x4*>(tile + 4 * v) = dv;
                    }
                }
                __syncthreads();
                if (fc < F)
                    for (int q = ch; q < np; q += nch) {
                        const float d = tile[q * F + fc], im = im_s[p0 + q];
                        fa1 += fabsf(d) * im;   // losses.py:200-201
                        fa2 += (d * d) * im;
                    }
                if (want_map) {
                    float s = 0.0f;
                    if (mp < np)
                        for (int j = 0; j < f_len; ++j) {
                            int jj = j + rot;
                            if (jj >= f_len) jj -= f_len;
                            const float d = tile[mp * F + f_lo + jj];
                            s += (a.map_kind == P4C_LOSS_MSE ? d * d : fabsf(d)) * w_s[f_lo + jj];
                        }
                    mq[mqi][mp] = s;
                }
                __syncthreads();
                if (want_map && tid < np) map_s[p0 + tid] += (mq[0][tid] + mq[1][tid]) + (mq[2][tid] + mq[3][tid]);
            }
            fred[0][tid] = fa1;
            fred[1][tid] = fa2;
            __syncthreads();
            if (tid < FP && tid < F) {
                float s1 = 0.0f, s2 = 0.0f;
                for (int c = 0; c < nch; ++c) {
                    s1 += fred[0][c * FP + tid];
                    s2 += fred[1][c * FP + tid];
                }
                const int64_t bt = (int64_t)b * a.T + t;
                a.partial[((0 * nbt + bt) * nblk + blockIdx.x) * F + tid] = s1;
                a.partial[((1 * nbt + bt) * nblk + blockIdx.x) * F + tid] = s2;
            }
        }
        if (want_map)   // (after the barrier above: every addition to map_s is in; the thread that reads i also zeroes i)
            for (int i = tid; i < n_cnt; i += 256) {
                const int64_t idx = (int64_t)t * a.N + n_begin + i;
                a.map_acc[idx] = a.accumulate ? a.map_acc[idx] + map_s[i] : map_s[i];
            }
    }
    __syncthreads();
    eval_store_count(any_s, n_cnt, MM, a.count_partial, cred);
}

// ------------------------------------------------------------------ scalar path (any alignment, F <= 256)
// lanes over the features of one or several grid points, as losses.hip::scaled_loss_partial_kernel; same ownership of grid points
__global__ void __launch_bounds__(256) eval_sums_scalar_kernel(EvalArgs a, int FP, int iters) {
    __shared__ float map_s[EV_MAX_R];
    __shared__ int any_s[EV_MAX_R];
    __shared__ float red[2][4][64 * EV_MAX_ITERS];
    __shared__ int cred[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, F = a.F, R = a.R;
    const int64_t nblk = gridDim.x, nbt = (int64_t)a.B * a.T;
    const int64_t n_begin = (int64_t)blockIdx.x * R;
    const int n_cnt = (int)((a.N - n_begin) < R ? (a.N - n_begin) : R);
    const bool want_map = a.map_acc != nullptr && a.map_kind != P4C_EVAL_MAP_NONE;
    const int PP = 64 / FP;
    const int pp = lane / FP, c0 = lane % FP;
    const unsigned long long segmask = (FP == 64) ? ~0ull : (((1ull << FP) - 1ull) << (pp * FP));
    float w[EV_MAX_ITERS];
#pragma unroll
    for (int it = 0; it < EV_MAX_ITERS; ++it) {
        const int f = c0 + it * FP;
        w[it] = (want_map && it < iters && f < F) ? a.weights[f] : 0.0f;
    }
    for (int i = tid; i < R; i += 256) any_s[i] = 0;
    for (int t = 0; t < a.T; ++t) {
        for (int i = tid; i < R; i += 256) map_s[i] = 0.0f;
        __syncthreads();
        for (int b = 0; b < a.B; ++b) {
            const float* p = a.pred + (int64_t)b * a.pred_bs + (int64_t)t * a.pred_ts;
            const float* g = a.target + (int64_t)b * a.tgt_bs + (int64_t)t * a.tgt_ts;
            const int64_t mbase = ((int64_t)b * a.T + t) * a.N * F;
            float a1[EV_MAX_ITERS], a2[EV_MAX_ITERS];
#pragma unroll
            for (int it = 0; it < EV_MAX_ITERS; ++it) a1[it] = a2[it] = 0.0f;
            // every lane of a wave runs the same number of iterations (ballot and shuffles need all lanes)
            for (int pb = wv * PP; pb < n_cnt; pb += 4 * PP) {
                const int q = pb + pp;
                const bool live = q < n_cnt;
                const int64_t n = n_begin + q;
                const float im = live ? a.interior[n] : 0.0f;
                float s = 0.0f;
                bool any_set = false;
#pragma unroll
                for (int it = 0; it < EV_MAX_ITERS; ++it) {
                    if (it < iters) {
                        const int f = c0 + it * FP;
                        bool set = false;
                        if (live && f < F) {
                            const int64_t e = n * F + f;
                            float tg = g[e], m = 1.0f;
                            if (a.mask_mode == P4C_MASK_FROM_NAN) {
                                const bool isn = tg != tg;
                                m = isn ? 0.0f : 1.0f;
                                if (isn) tg = 0.0f;
                            } else if (a.mask_mode == P4C_MASK_F32) {
                                m = ((const float*)a.mask)[mbase + e];
                            } else if (a.mask_mode == P4C_MASK_U8) {
                                m = ((const unsigned char*)a.mask)[mbase + e] ? 1.0f : 0.0f;
                            }
                            const float pm = p[e] * m, tm = tg * m;
                            const float d = pm - tm;
                            const float l1 = fabsf(d), l2 = d * d;
                            a1[it] += l1 * im;
                            a2[it] += l2 * im;
                            s += (a.map_kind == P4C_LOSS_MSE ? l2 : l1) * w[it];
                            set = m != 0.0f;
                        }
                        if (a.mask_mode != P4C_MASK_NONE) any_set = any_set || ((__ballot(set) & segmask) != 0ull);
                    }
                }
                s = seg_sum(s, FP);
                if (live && c0 == 0) {   // one lane per grid point, one wave per grid point: no race
                    if (want_map) map_s[q] += s;
                    if (any_set) any_s[q] = 1;
                }
            }
#pragma unroll
            for (int it = 0; it < EV_MAX_ITERS; ++it) {
                const float v1 = cross_seg_sum(a1[it], FP), v2 = cross_seg_sum(a2[it], FP);
                if (pp == 0) {
                    red[0][wv][it * 64 + c0] = v1;
                    red[1][wv][it * 64 + c0] = v2;
                }
            }
            __syncthreads();
            const int64_t bt = (int64_t)b * a.T + t;
            for (int i = tid; i < 2 * iters * FP; i += 256) {
                const int k = i / (iters * FP), j = i - k * iters * FP;
                const int it = j / FP, c = j - it * FP;
                const int f = c + it * FP;
                if (f < F) {
                    const int x = it * 64 + c;
                    a.partial[((k * nbt + bt) * nblk + blockIdx.x) * F + f] =
                        (red[k][0][x] + red[k][1][x]) + (red[k][2][x] + red[k][3][x]);
                }
            }
            __syncthreads();   // red is written again by the next slab
        }
        if (want_map)
            for (int i = tid; i < n_cnt; i += 256) {
                const int64_t idx = (int64_t)t * a.N + n_begin + i;
                a.map_acc[idx] = a.accumulate ? a.map_acc[idx] + map_s[i] : map_s[i];
            }
    }
    __syncthreads();
    eval_store_count(any_s, n_cnt, a.mask_mode, a.count_partial, cred);
}

// ------------------------------------------------------------------ finish
// grid: 2 * B*T workgroups, one per (kind, b, t).  Thread = (feature, chunk of the block partials); the chunks are added in order.
__global__ void __launch_bounds__(EV_FINAL_THREADS)
    eval_sums_final_kernel(const float* __restrict__ partial, const int32_t* __restrict__ count_partial, int64_t nblk,
                           float num_interior, const float* __restrict__ std, float* __restrict__ scores,
                           int32_t* __restrict__ masked_count, int nbt, int F, int FP, int has_mask) {
    __shared__ float red[EV_FINAL_THREADS];
    __shared__ int cred[EV_FINAL_THREADS / 64];
    const int tid = threadIdx.x;
    int cnt = 0;
    if (has_mask)
        for (int64_t i = tid; i < nblk; i += EV_FINAL_THREADS) cnt += count_partial[i];   // integers: exact in any order
    cnt = wave_sum_i(cnt);
    if ((tid & 63) == 0) cred[tid >> 6] = cnt;
    const int k = blockIdx.x / nbt, bt = blockIdx.x - k * nbt;
    const int fc = tid & (FP - 1), ch = tid / FP, nch = EV_FINAL_THREADS / FP;
    float s = 0.0f;
    if (fc < F) {
        const float* src = partial + ((int64_t)k * nbt + bt) * nblk * F + fc;
        for (int64_t blk = ch; blk < nblk; blk += nch) s += src[blk * F];
    }
    red[tid] = s;
    __syncthreads();
    int total = 0;
    for (int i = 0; i < EV_FINAL_THREADS / 64; ++i) total += cred[i];
    if (blockIdx.x == 0 && tid == 0) *masked_count = total;
    if (tid < FP && tid < F) {
        float tot = 0.0f;
        for (int c = 0; c < nch; ++c) tot += red[c * FP + tid];
        float v = tot / (num_interior - (float)total);   // losses.py:203
        if (k == 1) v = sqrtf(v);                        // losses.py:205-206
        scores[((int64_t)k * nbt + bt) * F + tid] = v * std[tid];
    }
}

static inline bool ev_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace p4c

using namespace p4c;

extern "C" size_t p4c_eval_sums_workspace_bytes(int B, int T, int64_t N, int F) {
    if (B < 1 || T < 1 || N < 1 || F < 1) return 0;
    const EvalGeom g = eval_geom(N);
    return ((size_t)2 * (size_t)B * (size_t)T * (size_t)F + 1) * (size_t)g.nblk * sizeof(float);
}

extern "C" int p4c_eval_sums(const float* pred, int64_t pred_bs, int64_t pred_ts, const float* target, int64_t tgt_bs,
                             int64_t tgt_ts, const void* mask, int mask_mode, const float* interior_mask, float num_interior,
                             const float* std, const float* weights, int map_kind, float* map_acc, int accumulate, float* scores,
                             int32_t* masked_count, void* workspace, int B, int T, int64_t N, int F, p4c_stream_t stream) {
    P4C_CHECK_ARG(pred && target && interior_mask && std && scores && masked_count && workspace, "p4c_eval_sums: null pointer");
    P4C_CHECK_ARG(B > 0 && T > 0 && N > 0 && F > 0 && F <= 64 * EV_MAX_ITERS, "p4c_eval_sums: bad dims (F=%d)", F);
    P4C_CHECK_ARG(mask_mode >= P4C_MASK_NONE && mask_mode <= P4C_MASK_U8, "p4c_eval_sums: bad mask mode");
    P4C_CHECK_ARG((mask_mode != P4C_MASK_F32 && mask_mode != P4C_MASK_U8) || mask, "p4c_eval_sums: null mask");
    P4C_CHECK_ARG(map_kind == P4C_LOSS_MSE || map_kind == P4C_LOSS_L1 || map_kind == P4C_EVAL_MAP_NONE,
                  "p4c_eval_sums: bad map kind");
    P4C_CHECK_ARG(map_kind == P4C_EVAL_MAP_NONE || !map_acc || weights, "p4c_eval_sums: the map needs weights");
    const EvalGeom geo = eval_geom(N);
    P4C_CHECK_ARG(geo.nblk <= 0x7fffffffLL, "p4c_eval_sums: N too large");
    EvalArgs a;
    a.pred = pred, a.pred_bs = pred_bs, a.pred_ts = pred_ts;
    a.target = target, a.tgt_bs = tgt_bs, a.tgt_ts = tgt_ts;
    a.mask = mask, a.mask_mode = mask_mode;
    a.interior = interior_mask, a.weights = weights;
    a.map_kind = map_kind, a.map_acc = map_kind == P4C_EVAL_MAP_NONE ? nullptr : map_acc, a.accumulate = accumulate;
    a.partial = (float*)workspace;
    a.count_partial = (int32_t*)((float*)workspace + (size_t)2 * B * T * F * geo.nblk);
    a.B = B, a.T = T, a.N = N, a.F = F, a.R = geo.R;
    const bool explicit_mask = mask_mode == P4C_MASK_F32 || mask_mode == P4C_MASK_U8;
    const bool flat = F <= 64 && (N * F) % 4 == 0 && pred_bs % 4 == 0 && pred_ts % 4 == 0 && tgt_bs % 4 == 0 && tgt_ts % 4 == 0 &&
                      ev_aligned16(pred) && ev_aligned16(target) && (!explicit_mask || ev_aligned16(mask));
    if (flat) {
        const unsigned rcp = ((1u << 20) + F - 1) / F;
        const dim3 grid((unsigned)geo.nblk);
        const int FP = pow2_ge(F, 64);
        switch (mask_mode) {
            case P4C_MASK_FROM_NAN: hipLaunchKernelGGL(eval_sums_flat_kernel<P4C_MASK_FROM_NAN>, grid, dim3(256), 0, as_stream(stream), a, rcp, FP); break;
            case P4C_MASK_F32: hipLaunchKernelGGL(eval_sums_flat_kernel<P4C_MASK_F32>, grid, dim3(256), 0, as_stream(stream), a, rcp, FP); break;
            case P4C_MASK_U8: hipLaunchKernelGGL(eval_sums_flat_kernel<P4C_MASK_U8>, grid, dim3(256), 0, as_stream(stream), a, rcp, FP); break;
            default: hipLaunchKernelGGL(eval_sums_flat_kernel<P4C_MASK_NONE>, grid, dim3(256), 0, as_stream(stream), a, rcp, FP); break;
        }
    } else {
        const int FP = pow2_ge(F, 64), iters = (F + FP - 1) / FP;
        hipLaunchKernelGGL(eval_sums_scalar_kernel, dim3((unsigned)geo.nblk), dim3(256), 0, as_stream(stream), a, FP, iters);
    }
    P4C_CHECK_LAUNCH("p4c_eval_sums(partial)");
    hipLaunchKernelGGL(eval_sums_final_kernel, dim3(2 * B * T), dim3(EV_FINAL_THREADS), 0, as_stream(stream),
                       (const float*)a.partial, (const int32_t*)a.count_partial, geo.nblk, num_interior, std, scores,
                       masked_count, B * T, F, pow2_ge(F, 256), mask_mode != P4C_MASK_NONE ? 1 : 0);
    P4C_CHECK_LAUNCH("p4c_eval_sums(final)");
    return P4C_OK;
}
