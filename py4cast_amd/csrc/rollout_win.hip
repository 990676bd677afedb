// The AR step on an auto-padded grid: build_x and the fused update / loss step (forward, free step, backward) with the NETWORK side
// (x, y, dy, dx) on the padded grid (B, Hp, Wp, channels) and the STATE side (previous / new state, target, statics, forcing, masks,
// dprev, g_next) dense at (B, H, W, ..) -- mfai's AutoPaddingModel (pad -> network -> crop, lightning.py:591-596) as addressing:
//   state pixel (h, w)  <->  network row (top + h) * Wp + left + w
// Nothing is copied, padded or cropped.  Outside the window x is +0.0 in every channel (the reference's zero pad) and dy is +0.0
// (a cropped output has no gradient); both are written in EVERY element, so no memset runs ahead of them.
//
// Streaming, HBM-bound passes: no LDS, no MFMA.  One lane per (pixel, feature quad) with 16-byte accesses where the feature count and
// the alignments allow it, one lane per (pixel, feature) otherwise (F = 21, the NaN mask channel of build_x; the backward always keeps
// its quads on the dy / dx rows and, at such an F, reads the state side element by element).  The kernels that write a
// network-side tensor walk the padded pixels and decide inside / outside once per pixel; the forward steps walk the state pixels.
//
// Compiled with -ffp-contract=off like losses.hip / rollout.hip: the element arithmetic below is that of losses.hip's
// ar_update_loss_{fwd,bwd}[_v4]_kernel restated in the same order, so new state, dy and dprev are those kernels' bits (fed the cropped
// rows); the loss column goes through the same workspace (p4c_loss_workspace_bytes) and the same final kernel.
#include <limits.h>

#include "common.hpp"

namespace p4c {

// losses.hip: out[b * out_stride] = sum(partials of b) / (num_interior - masked)
__global__ void __launch_bounds__(64) weighted_loss_final_kernel(const float* __restrict__ partial, int nblk, float num_interior,
                                                                 const int32_t* __restrict__ masked_count,
                                                                 float* __restrict__ out, int64_t out_stride, int nbt);

namespace win {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v4f_a4 __attribute__((ext_vector_type(4), aligned(4)));  // 4-byte aligned 16-byte access (forcing rows)

constexpr int MAX_ITERS = 4;     // channels per lane of the scalar kernels: rows of at most 256 channels
constexpr int MAX_BLOCKS = 512;  // partial blocks per sample, as losses.hip's LOSS_MAX_BLOCKS (step_fwd_win checks the workspace's size)

struct Window {
    int H, W, Hp, Wp, top, left;
    // network row of state pixel n
    __device__ __forceinline__ int net_row(int n) const {
        const int h = (int)((unsigned)n / (unsigned)W), w = n - h * W;
        return (top + h) * Wp + left + w;
    }
    // state pixel of network row np; false outside the window
    __device__ __forceinline__ bool state_pixel(int np, int& n) const {
        const int hp = (int)((unsigned)np / (unsigned)Wp), wp = np - hp * Wp;
        const int h = hp - top, w = wp - left;
        n = h * W + w;
        return (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
    }
};

__host__ __device__ static inline int pow2_ge64(int v) {
    int p = 1;
    while (p < v && p < 64) p <<= 1;
    return p;
}

// losses.hip loss_elem / loss_elem_grad
__device__ __forceinline__ float loss_elem(float pred, float tgt, float m, int kind) {
    const float pm = pred * m, tm = tgt * m;
    const float d = pm - tm;
    return kind == P4C_LOSS_MSE ? d * d : fabsf(d);
}
__device__ __forceinline__ float loss_elem_grad(float pred, float tgt, float m, int kind) {
    const float d = pred * m - tgt * m;
    if (kind == P4C_LOSS_MSE) return 2.0f * d * m;
    return (d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.0f)) * m;
}

// ------------------------------------------------------------------ build_x through the window
// grid (nblk, B); a wave takes PP = 64 / FP network rows per pass, lane % FP = channel (+ it * FP)
template <typename TX>
__global__ void __launch_bounds__(256)
    build_x_win_kernel(const float* __restrict__ prev, int64_t prev_bs, const float* __restrict__ statics, int64_t statics_bs,
                       const float* __restrict__ forcing, int64_t forcing_bs, TX* __restrict__ x, int c_pad, int F, int Fs, int Ff,
                       int mask_on_nan, int FP, int iters, Window g) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int PP = 64 / FP;
    const int pp = lane / FP, c0 = lane % FP;
    const int o_stat = F, o_forc = F + Fs, o_mask = F + Fs + Ff;
    const int c_in = o_mask + (mask_on_nan ? 1 : 0);
    const int NP = g.Hp * g.Wp;
    const unsigned long long segmask = (FP == 64) ? ~0ull : (((1ull << FP) - 1ull) << (pp * FP));
    const int64_t stride = (int64_t)gridDim.x * 4 * PP;
    // (the bound is on the wave's first row: every lane of a wave takes part in the ballots)
    for (int64_t base = ((int64_t)blockIdx.x * 4 + wv) * PP; base < NP; base += stride) {
        const int np = (int)base + pp;
        int n = 0;
        const bool live = np < NP;
        const bool inside = live && g.state_pixel(np, n);
        float vals[MAX_ITERS];
        bool any_nan = false;
#pragma unroll
        for (int it = 0; it < MAX_ITERS; ++it) {
            if (it >= iters) break;
            const int c = c0 + it * FP;
            float v = 0.0f;
            bool counts = false;  // channel takes part in the NaN union (state + forcing only)
            if (inside && c < c_pad) {
                if (c < o_stat) {
                    v = prev[(int64_t)b * prev_bs + (int64_t)n * F + c];
                    counts = true;
                } else if (c < o_forc) {
                    v = statics[(int64_t)b * statics_bs + (int64_t)n * Fs + (c - o_stat)];
                } else if (c < o_mask) {
                    v = forcing[(int64_t)b * forcing_bs + (int64_t)n * Ff + (c - o_forc)];
                    counts = true;
                }
            }
            vals[it] = v;
            if (mask_on_nan) {
                const bool isn = counts && (v != v);
                const unsigned long long bal = __ballot(isn);
                any_nan = any_nan || ((bal & segmask) != 0ull);
                if (isn) vals[it] = 0.0f;
            }
        }
        if (!live) continue;
        TX* xrow = x + ((int64_t)b * NP + np) * c_pad;
#pragma unroll
        for (int it = 0; it < MAX_ITERS; ++it) {
            if (it >= iters) break;
            const int c = c0 + it * FP;
            if (c < c_pad) {
                float v = vals[it];
                if (mask_on_nan && inside && c == c_in - 1) v = any_nan ? 0.0f : 1.0f;
                xrow[c] = from_f32<TX>(v);
            }
        }
    }
}

// 16-byte form (no NaN mask channel, c_pad % 4 == 0): a lane produces one quad of the output row.  The quad's source is classified
// once, as in rollout.hip's build_x_v4_kernel: kind 0 = 16 bytes of one source, 1 = the last 1..3 forcing values, 2 = zero padding,
// 3 = a quad that straddles two sources (or an unaligned source): gathered element by element.
template <typename TX>
__global__ void __launch_bounds__(256)
    build_x_win_v4_kernel(const float* __restrict__ prev, int64_t prev_bs, const float* __restrict__ statics, int64_t statics_bs,
                          const float* __restrict__ forcing, int64_t forcing_bs, TX* __restrict__ x, int c_pad, int F, int Fs, int Ff,
                          int FP4, int vec_prev, int vec_stat, Window g) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int PP = 64 / FP4;
    const int pp = lane / FP4, q = lane % FP4;
    const int c0 = 4 * q;
    if (c0 >= c_pad) return;
    const int o_stat = F, o_forc = F + Fs, c_in = F + Fs + Ff;
    const int NP = g.Hp * g.Wp;
    int kind = 3, nvalid = 0;
    const float* src = nullptr;
    int64_t rstride = 0;
    if (c0 >= c_in) {
        kind = 2;
    } else if (c0 + 3 < o_stat) {
        if (vec_prev) { kind = 0; src = prev + (int64_t)b * prev_bs + c0; rstride = F; }
    } else if (c0 >= o_stat && c0 + 3 < o_forc) {
        if (vec_stat) { kind = 0; src = statics + (int64_t)b * statics_bs + (c0 - o_stat); rstride = Fs; }
    } else if (c0 >= o_forc) {
        src = forcing + (int64_t)b * forcing_bs + (c0 - o_forc);
        rstride = Ff;
        nvalid = c_in - c0 < 4 ? c_in - c0 : 4;
        kind = nvalid == 4 ? 0 : 1;
    }
    const int64_t stride = (int64_t)gridDim.x * 4 * PP;
    for (int64_t i = ((int64_t)blockIdx.x * 4 + wv) * PP + pp; i < NP; i += stride) {
        const int np = (int)i;
        int n;
        v4f v = {0.f, 0.f, 0.f, 0.f};
        if (g.state_pixel(np, n)) {
            if (kind == 0) {
                v = *reinterpret_cast<const v4f_a4*>(src + (int64_t)n * rstride);
            } else if (kind == 1) {
                const float* p = src + (int64_t)n * rstride;
                v[0] = p[0];
                if (nvalid > 1) v[1] = p[1];
                if (nvalid > 2) v[2] = p[2];
            } else if (kind == 3) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + j;
                    float e = 0.f;
                    if (c < o_stat) e = prev[(int64_t)b * prev_bs + (int64_t)n * F + c];
                    else if (c < o_forc) e = statics[(int64_t)b * statics_bs + (int64_t)n * Fs + (c - o_stat)];
                    else if (c < c_in) e = forcing[(int64_t)b * forcing_bs + (int64_t)n * Ff + (c - o_forc)];
                    v[j] = e;
                }
            }
        }
        store4f(x + ((int64_t)b * NP + np) * c_pad + c0, v);
    }
}

// ------------------------------------------------------------------ forward step: y read through the window
// grid (nblk, B); walks the STATE pixels.  LOSS = false: the free step (no weights, no partials; target / interior_mask only where a
// border is forced).  The loop bodies are losses.hip's ar_update_loss_fwd_v4_kernel / ar_update_loss_fwd_kernel.
template <typename TY, bool LOSS>
__global__ void __launch_bounds__(256)
    step_fwd_win_v4_kernel(const float* __restrict__ prev, int64_t prev_bs, const TY* __restrict__ y, int y_cs,
                           const float* __restrict__ target, int64_t tgt_bs, const float* __restrict__ std,
                           const float* __restrict__ mean, const float* __restrict__ border_mask,
                           const float* __restrict__ interior_mask, float* __restrict__ new_state, int64_t new_bs,
                           const float* __restrict__ weights, int kind, int mask_mode, float* __restrict__ partial, int N, int F,
                           float keep_prev, int FP4, Window g) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int PP = 64 / FP4;
    const int pp = lane / FP4, q = lane % FP4;
    const bool act = 4 * q < F;
    const bool from_nan = mask_mode == P4C_MASK_FROM_NAN;
    const int64_t NP = (int64_t)g.Hp * g.Wp;
    v4f w = {0, 0, 0, 0}, sd = {1, 1, 1, 1}, mn = {0, 0, 0, 0};
    if (act) {
        if (LOSS) w = *reinterpret_cast<const v4f*>(weights + 4 * q);
        if (std) {
            sd = *reinterpret_cast<const v4f*>(std + 4 * q);
            mn = *reinterpret_cast<const v4f*>(mean + 4 * q);
        }
    }
    float acc = 0.0f;
    const int64_t stride = (int64_t)gridDim.x * 4 * PP;
    for (int64_t i = ((int64_t)blockIdx.x * 4 + wv) * PP + pp; i < N; i += stride) {
        if (!act) continue;
        const int n = (int)i;
        const float im = (LOSS || border_mask) ? interior_mask[n] : 1.0f;
        const float bm = border_mask ? border_mask[n] : 0.0f;
        const int64_t e = (int64_t)n * F + 4 * q;
        const v4f yv = load4f(y + ((int64_t)b * NP + g.net_row(n)) * y_cs + 4 * q);
        v4f pv = {0, 0, 0, 0};
        if (prev) pv = *reinterpret_cast<const v4f*>(prev + (int64_t)b * prev_bs + e);
        v4f tg = {0, 0, 0, 0};
        if (LOSS || border_mask) tg = *reinterpret_cast<const v4f*>(target + (int64_t)b * tgt_bs + e);
        v4f o;
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float p0 = pv[j], t0 = tg[j], m = 1.0f;
            if (from_nan) {
                p0 = nan_to_zero(p0);
                m = (t0 != t0) ? 0.0f : 1.0f;
                t0 = nan_to_zero(t0);
            }
            float pr;
            if (std) {
                pr = p0 * keep_prev + yv[j] * sd[j];
                pr = pr + mn[j];
            } else {
                pr = p0 * keep_prev + yv[j];
            }
            if (border_mask) pr = bm * t0 + im * pr;
            o[j] = pr;
            if (LOSS) s += loss_elem(pr, t0, m, kind) * w[j];
        }
        *reinterpret_cast<v4f*>(new_state + (int64_t)b * new_bs + e) = o;
        if (LOSS) acc += s * im;
    }
    if (!LOSS) return;
    acc = wave_sum(acc);
    if (lane == 0) red[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one lane per (pixel, feature): F <= 64
template <typename TY, bool LOSS>
__global__ void __launch_bounds__(256)
    step_fwd_win_kernel(const float* __restrict__ prev, int64_t prev_bs, const TY* __restrict__ y, int y_cs,
                        const float* __restrict__ target, int64_t tgt_bs, const float* __restrict__ std,
                        const float* __restrict__ mean, const float* __restrict__ border_mask,
                        const float* __restrict__ interior_mask, float* __restrict__ new_state, int64_t new_bs,
                        const float* __restrict__ weights, int kind, int mask_mode, float* __restrict__ partial, int N, int F,
                        float keep_prev, int FP, Window g) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int PP = 64 / FP;
    const int pp = lane / FP, f = lane % FP;
    const bool act = f < F;
    const bool from_nan = mask_mode == P4C_MASK_FROM_NAN;
    const int64_t NP = (int64_t)g.Hp * g.Wp;
    const float w = (LOSS && act) ? weights[f] : 0.0f;
    const float sd = (act && std) ? std[f] : 1.0f;
    const float mn = (act && mean) ? mean[f] : 0.0f;
    float acc = 0.0f;
    const int64_t stride = (int64_t)gridDim.x * 4 * PP;
    for (int64_t i = ((int64_t)blockIdx.x * 4 + wv) * PP + pp; i < N; i += stride) {
        if (!act) continue;
        const int n = (int)i;
        const float im = (LOSS || border_mask) ? interior_mask[n] : 1.0f;
        const float bm = border_mask ? border_mask[n] : 0.0f;
        const int64_t e = (int64_t)n * F + f;
        const float yv = to_f32<TY>(y[((int64_t)b * NP + g.net_row(n)) * y_cs + f]);
        float pv = 0.0f;
        if (prev) {
            pv = prev[(int64_t)b * prev_bs + e];
            if (from_nan) pv = nan_to_zero(pv);
        }
        float tg = (LOSS || border_mask) ? target[(int64_t)b * tgt_bs + e] : 0.0f;
        float m = 1.0f;
        if (from_nan) {
            m = (tg != tg) ? 0.0f : 1.0f;
            tg = nan_to_zero(tg);
        }
        float pr;
        if (std) {
            pr = pv * keep_prev + yv * sd;
            pr = pr + mn;
        } else {
            pr = pv * keep_prev + yv;
        }
        if (border_mask) pr = bm * tg + im * pr;
        new_state[(int64_t)b * new_bs + e] = pr;
        if (LOSS) {
            const float s = loss_elem(pr, tg, m, kind) * w;
            acc += s * im;
        }
    }
    if (!LOSS) return;
    acc = wave_sum(acc);
    if (lane == 0) red[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------------ backward step: dx read, dy written through the window
// grid (nblk, B); walks the NETWORK rows: every element of dy is written (zeros outside the window and in channels >= F).
// The loop body is losses.hip's ar_update_loss_bwd_v4_kernel (not SAVED, LOSS).
// A lane owns 4 channels of a dy / dx row (16-byte or, bf16, 8-byte accesses).  ALIGNED: F % 4 == 0 and 16-byte aligned state rows --
// the state side in 16-byte pieces too.  Otherwise (F = 21: rows of 84 bytes) the state side goes element by element, up to F.
template <typename TY, bool ALIGNED>
__global__ void __launch_bounds__(256)
    step_bwd_win_v4_kernel(const float* __restrict__ g_next, int64_t g_next_bs, const TY* __restrict__ g_next2, int g2_cs,
                           const float* __restrict__ gloss, int64_t gloss_stride, const float* __restrict__ new_state,
                           int64_t new_bs, const float* __restrict__ target, int64_t tgt_bs, const float* __restrict__ std,
                           const float* __restrict__ interior_mask, int force_border, const float* __restrict__ weights,
                           float num_interior, const int32_t* __restrict__ masked_count, int kind, int mask_mode,
                           TY* __restrict__ dy, int y_cs, float* dprev, int64_t dprev_bs, int F, float keep_prev, int FP4, Window g) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int PP = 64 / FP4;
    const int pp = lane / FP4, q = lane % FP4;
    const bool act = 4 * q < F, wr = 4 * q < y_cs;
    if (!wr) return;
    const bool from_nan = mask_mode == P4C_MASK_FROM_NAN;
    const int NP = g.Hp * g.Wp;
    const float denom = num_interior - (masked_count ? (float)(*masked_count) : 0.0f);
    const float scale = gloss ? gloss[(int64_t)b * gloss_stride] / denom : 0.0f;
    const int nf = ALIGNED ? 4 : (F - 4 * q < 4 ? F - 4 * q : 4);   // features of this lane's quad (<= 0: none)
    v4f w = {0, 0, 0, 0}, sd = {1, 1, 1, 1};
    if (act) {
        if (ALIGNED) {
            w = *reinterpret_cast<const v4f*>(weights + 4 * q);
            if (std) sd = *reinterpret_cast<const v4f*>(std + 4 * q);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nf) {
                    w[j] = weights[4 * q + j];
                    if (std) sd[j] = std[4 * q + j];
                }
        }
    }
    const int64_t stride = (int64_t)gridDim.x * 4 * PP;
    for (int64_t i = ((int64_t)blockIdx.x * 4 + wv) * PP + pp; i < NP; i += stride) {
        const int np = (int)i;
        const int64_t row = (int64_t)b * NP + np;
        int n;
        v4f gy = {0, 0, 0, 0};
        if (act && g.state_pixel(np, n)) {
            const float im = interior_mask[n];
            const float sc = scale * im;
            const float blend = force_border ? im : 1.0f;
            const int64_t e = (int64_t)n * F + 4 * q;
            v4f ns = {0, 0, 0, 0}, tg = {0, 0, 0, 0}, g1 = {0, 0, 0, 0}, g2 = {0, 0, 0, 0};
            if (ALIGNED) {
                ns = *reinterpret_cast<const v4f*>(new_state + (int64_t)b * new_bs + e);
                tg = *reinterpret_cast<const v4f*>(target + (int64_t)b * tgt_bs + e);
                if (g_next) g1 = *reinterpret_cast<const v4f*>(g_next + (int64_t)b * g_next_bs + e);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nf) {
                        ns[j] = new_state[(int64_t)b * new_bs + e + j];
                        tg[j] = target[(int64_t)b * tgt_bs + e + j];
                        if (g_next) g1[j] = g_next[(int64_t)b * g_next_bs + e + j];
                    }
            }
            if (g_next2) g2 = load4f(g_next2 + row * g2_cs + 4 * q);
            v4f gp = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!ALIGNED && j >= nf) continue;   // channels F .. of the quad that straddles F: dy = +0.0
                float t0 = tg[j], m = 1.0f;
                if (from_nan) {
                    m = (t0 != t0) ? 0.0f : 1.0f;
                    t0 = nan_to_zero(t0);
                }
                float gg = sc * w[j] * loss_elem_grad(ns[j], t0, m, kind);
                if (g_next) gg += g1[j];
                if (g_next2) gg += g2[j];
                gp[j] = gg * blend;
                gy[j] = std ? gp[j] * sd[j] : gp[j];
            }
            if (dprev) {
                if (ALIGNED) {
                    *reinterpret_cast<v4f*>(dprev + (int64_t)b * dprev_bs + e) = gp * keep_prev;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < nf) dprev[(int64_t)b * dprev_bs + e + j] = gp[j] * keep_prev;
                }
            }
        }
        store4f(dy + row * y_cs + 4 * q, gy);
    }
}

// blocks per sample of a kernel whose waves take PP pixels per pass: the rule of losses.hip's loss_blocks -- about 8 blocks per CU
// over all samples, at most MAX_BLOCKS (the loss workspace holds that many partials per sample); the kernels grid-stride the rest
static inline int blocks_per_sample(int64_t pixels, int PP, int B) {
    int64_t blocks = ((pixels + PP - 1) / PP + 3) / 4;
    int64_t cap = ((int64_t)num_cus() * 8 + B - 1) / B;
    if (cap < 1) cap = 1;
    if (blocks > cap) blocks = cap;
    if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool rows_dtype(int dtype) { return dtype == P4C_F32 || dtype == P4C_BF16; }

static int check_window(const char* who, int64_t N, const Window& g) {
    P4C_CHECK_ARG(g.H > 0 && g.W > 0 && (int64_t)g.H * g.W == N, "%s: H * W (%d * %d) != N (%lld)", who, g.H, g.W, (long long)N);
    P4C_CHECK_ARG(g.top >= 0 && g.left >= 0 && g.Hp > 0 && g.Wp > 0 && (int64_t)g.top + g.H <= g.Hp && (int64_t)g.left + g.W <= g.Wp,
                  "%s: the window (%d + %d, %d + %d) does not fit the padded grid %d x %d", who, g.top, g.H, g.left, g.W, g.Hp, g.Wp);
    P4C_CHECK_ARG((int64_t)g.Hp * g.Wp <= INT_MAX / 2, "%s: padded grid too large", who);   // (pixel indices are 32-bit)
    return P4C_OK;
}

struct StepFwdWin {
    const float* prev; int64_t prev_bs; const void* y; int y_dtype; int y_cs;
    const float* target; int64_t tgt_bs; const float* std; const float* mean; const float* border_mask; const float* interior_mask;
    float* new_state; int64_t new_bs;
    const float* weights; float num_interior; const int32_t* masked_count; int kind; int mask_mode;
    float* loss_out; int64_t loss_stride; void* workspace;
    int B; int64_t N; int F; float keep_prev;
    Window g; bool loss; p4c_stream_t stream;
};

static int step_fwd_win(const StepFwdWin& s, const char* who) {
    P4C_CHECK_ARG(s.B > 0 && s.N > 0, "%s: bad dims", who);
    P4C_TRY(check_window(who, s.N, s.g));
    if (s.loss)
        P4C_CHECK_ARG(s.y && s.target && s.interior_mask && s.new_state && s.weights && s.loss_out && s.workspace, "%s: null pointer", who);
    else
        P4C_CHECK_ARG(s.y && s.new_state && (!s.border_mask || (s.target && s.interior_mask)),
                      "%s: null pointer (border forcing needs border_mask, interior_mask and target)", who);
    P4C_CHECK_ARG(s.prev || s.keep_prev == 0.0f, "%s: prev is null but keep_prev != 0", who);
    P4C_CHECK_ARG((s.std == nullptr) == (s.mean == nullptr), "%s: std and mean go together", who);
    P4C_CHECK_ARG(s.mask_mode == P4C_MASK_NONE || s.mask_mode == P4C_MASK_FROM_NAN, "%s: only MASK_NONE / MASK_FROM_NAN are fused", who);
    P4C_CHECK_ARG(s.F > 0 && s.F <= 64 && s.y_cs >= s.F, "%s: bad F / y_cs (F <= 64)", who);
    P4C_CHECK_ARG(rows_dtype(s.y_dtype), "%s: bad dtype %d", who, s.y_dtype);
    const bool v4 = s.F % 4 == 0 && s.y_cs % 4 == 0 && s.prev_bs % 4 == 0 && s.tgt_bs % 4 == 0 && s.new_bs % 4 == 0 && aligned16(s.prev) &&
                    aligned16(s.target) && aligned16(s.new_state) && aligned16(s.y) && (!s.loss || aligned16(s.weights)) &&
                    aligned16(s.std) && aligned16(s.mean);
    const int FP = v4 ? pow2_ge64(s.F / 4) : pow2_ge64(s.F);
    const int nblk = blocks_per_sample(s.N, 64 / FP, s.B);
    // the partials go to the workspace losses.hip sizes: one float per block and sample must fit what it hands out
    if (s.loss)
        P4C_CHECK_ARG((size_t)nblk * (size_t)s.B * sizeof(float) <= p4c_loss_workspace_bytes(s.B, 1, s.N, 1),
                      "%s: %d blocks per sample exceed the loss workspace", who, nblk);
    const dim3 grid(nblk, s.B), block(256);
    hipStream_t st = as_stream(s.stream);
#define P4C_WIN_FWD(KERNEL, TY, LOSS)                                                                                                   \
    hipLaunchKernelGGL((KERNEL<TY, LOSS>), grid, block, 0, st, s.prev, s.prev_bs, (const TY*)s.y, s.y_cs, s.target, s.tgt_bs, s.std, s.mean, \
                       s.border_mask, s.interior_mask, s.new_state, s.new_bs, s.weights, s.kind, s.mask_mode, (float*)s.workspace,      \
                       (int)s.N, s.F, s.keep_prev, FP, s.g)
    if (v4) {
        if (s.y_dtype == P4C_F32) { if (s.loss) P4C_WIN_FWD(step_fwd_win_v4_kernel, float, true); else P4C_WIN_FWD(step_fwd_win_v4_kernel, float, false); }
        else { if (s.loss) P4C_WIN_FWD(step_fwd_win_v4_kernel, bf16, true); else P4C_WIN_FWD(step_fwd_win_v4_kernel, bf16, false); }
    } else {
        if (s.y_dtype == P4C_F32) { if (s.loss) P4C_WIN_FWD(step_fwd_win_kernel, float, true); else P4C_WIN_FWD(step_fwd_win_kernel, float, false); }
        else { if (s.loss) P4C_WIN_FWD(step_fwd_win_kernel, bf16, true); else P4C_WIN_FWD(step_fwd_win_kernel, bf16, false); }
    }
#undef P4C_WIN_FWD
    P4C_CHECK_LAUNCH(who);
    if (!s.loss) return P4C_OK;
    hipLaunchKernelGGL(weighted_loss_final_kernel, dim3(s.B), dim3(64), 0, st, (const float*)s.workspace, nblk, s.num_interior,
                       s.masked_count, s.loss_out, s.loss_stride, s.B);
    P4C_CHECK_LAUNCH("p4c_ar_update_loss_fwd_win(final)");
    return P4C_OK;
}

}  // namespace win
}  // namespace p4c

using namespace p4c;
using namespace p4c::win;

extern "C" int p4c_build_x_win(const float* prev, int64_t prev_bs, int64_t prev_ts, const float* statics, int64_t statics_bs,
                               const float* forcing, int64_t forcing_bs, void* x, int x_dtype, int c_pad, int B, int T_in, int64_t N,
                               int F, int Fs, int Ff, int mask_on_nan, int downscaling_only, int H, int W, int Hp, int Wp, int top,
                               int left, p4c_stream_t stream) {
    (void)prev_ts;
    const char* who = "p4c_build_x_win";
    P4C_CHECK_ARG(x && prev && statics && forcing, "%s: null pointer", who);
    P4C_CHECK_ARG(T_in == 1 && !downscaling_only, "%s: one input state only (T_in = %d), no downscaling_only", who, T_in);
    P4C_CHECK_ARG(B > 0 && N > 0 && F > 0 && Fs >= 0 && Ff >= 0, "%s: bad dims", who);
    const Window g{H, W, Hp, Wp, top, left};
    P4C_TRY(check_window(who, N, g));
    const int c_in = F + Fs + Ff + (mask_on_nan ? 1 : 0);
    P4C_CHECK_ARG(c_pad >= c_in, "%s: c_pad (%d) < C_in (%d)", who, c_pad, c_in);
    P4C_CHECK_ARG(c_pad <= 64 * MAX_ITERS, "%s: c_pad %d too large (max %d)", who, c_pad, 64 * MAX_ITERS);
    P4C_CHECK_ARG(rows_dtype(x_dtype), "%s: bad dtype %d", who, x_dtype);
    const int64_t NP = (int64_t)Hp * Wp;
    hipStream_t st = as_stream(stream);
    if (!mask_on_nan && c_pad % 4 == 0 && aligned16(x)) {
        const int FP4 = pow2_ge64(c_pad / 4);
        const int vec_prev = F % 4 == 0 && prev_bs % 4 == 0 && aligned16(prev);
        const int vec_stat = Fs % 4 == 0 && F % 4 == 0 && statics_bs % 4 == 0 && aligned16(statics);
        const dim3 grid(blocks_per_sample(NP, 64 / FP4, B), B);
        if (x_dtype == P4C_F32)
            hipLaunchKernelGGL(build_x_win_v4_kernel<float>, grid, dim3(256), 0, st, prev, prev_bs, statics, statics_bs, forcing, forcing_bs,
                               (float*)x, c_pad, F, Fs, Ff, FP4, vec_prev, vec_stat, g);
        else
            hipLaunchKernelGGL(build_x_win_v4_kernel<bf16>, grid, dim3(256), 0, st, prev, prev_bs, statics, statics_bs, forcing, forcing_bs,
                               (bf16*)x, c_pad, F, Fs, Ff, FP4, vec_prev, vec_stat, g);
        P4C_CHECK_LAUNCH("p4c_build_x_win(v4)");
        return P4C_OK;
    }
    const int FP = pow2_ge64(c_pad), iters = (c_pad + FP - 1) / FP;
    const dim3 grid(blocks_per_sample(NP, 64 / FP, B), B);
    if (x_dtype == P4C_F32)
        hipLaunchKernelGGL(build_x_win_kernel<float>, grid, dim3(256), 0, st, prev, prev_bs, statics, statics_bs, forcing, forcing_bs,
                           (float*)x, c_pad, F, Fs, Ff, mask_on_nan, FP, iters, g);
    else
        hipLaunchKernelGGL(build_x_win_kernel<bf16>, grid, dim3(256), 0, st, prev, prev_bs, statics, statics_bs, forcing, forcing_bs,
                           (bf16*)x, c_pad, F, Fs, Ff, mask_on_nan, FP, iters, g);
    P4C_CHECK_LAUNCH(who);
    return P4C_OK;
}

extern "C" int p4c_ar_update_loss_fwd_win(const float* prev, int64_t prev_bs, const void* y, int y_dtype, int y_cs, const float* target,
                                          int64_t tgt_bs, const float* std, const float* mean, const float* border_mask,
                                          const float* interior_mask, float* new_state, int64_t new_bs, const float* weights,
                                          float num_interior, const int32_t* masked_count, int kind, int mask_mode, float* loss_out,
                                          int64_t loss_stride, void* workspace, int B, int64_t N, int F, float keep_prev, int H, int W,
                                          int Hp, int Wp, int top, int left, p4c_stream_t stream) {
    return step_fwd_win(StepFwdWin{prev, prev_bs, y, y_dtype, y_cs, target, tgt_bs, std, mean, border_mask, interior_mask, new_state, new_bs,
                                   weights, num_interior, masked_count, kind, mask_mode, loss_out, loss_stride, workspace, B, N, F,
                                   keep_prev, Window{H, W, Hp, Wp, top, left}, true, stream},
                        "p4c_ar_update_loss_fwd_win");
}

extern "C" int p4c_ar_update_next_win(const float* prev, int64_t prev_bs, const void* y, int y_dtype, int y_cs, const float* target,
                                      int64_t tgt_bs, const float* std, const float* mean, const float* border_mask,
                                      const float* interior_mask, float* new_state, int64_t new_bs, int nan_to_num, int B, int64_t N,
                                      int F, float keep_prev, int H, int W, int Hp, int Wp, int top, int left, p4c_stream_t stream) {
    P4C_CHECK_ARG((target == nullptr) == (border_mask == nullptr), "p4c_ar_update_next_win: target and border_mask go together");
    return step_fwd_win(StepFwdWin{prev, prev_bs, y, y_dtype, y_cs, target, tgt_bs, std, mean, border_mask, interior_mask, new_state, new_bs,
                                   nullptr, 0.0f, nullptr, P4C_LOSS_MSE, nan_to_num ? P4C_MASK_FROM_NAN : P4C_MASK_NONE, nullptr, 0,
                                   nullptr, B, N, F, keep_prev, Window{H, W, Hp, Wp, top, left}, false, stream},
                        "p4c_ar_update_next_win");
}

extern "C" int p4c_ar_update_loss_bwd_win(const float* g_next, int64_t g_next_bs, const void* g_next2, int g2_dtype, int g2_cs,
                                          const float* gloss, int64_t gloss_stride, const float* new_state, int64_t new_bs,
                                          const float* target, int64_t tgt_bs, const float* std, const float* interior_mask,
                                          int force_border, const float* weights, float num_interior, const int32_t* masked_count,
                                          int kind, int mask_mode, void* dy, int dy_dtype, int y_cs, float* dprev, int64_t dprev_bs,
                                          int B, int64_t N, int F, float keep_prev, int H, int W, int Hp, int Wp, int top, int left,
                                          p4c_stream_t stream) {
    const char* who = "p4c_ar_update_loss_bwd_win";
    P4C_CHECK_ARG(B > 0 && N > 0, "%s: bad dims", who);
    const Window g{H, W, Hp, Wp, top, left};
    P4C_TRY(check_window(who, N, g));
    P4C_CHECK_ARG(new_state && target && interior_mask && weights && dy, "%s: null pointer", who);
    P4C_CHECK_ARG(mask_mode == P4C_MASK_NONE || mask_mode == P4C_MASK_FROM_NAN, "%s: only MASK_NONE / MASK_FROM_NAN are fused", who);
    P4C_CHECK_ARG(F > 0 && F <= 64 && y_cs >= F && y_cs <= 256, "%s: bad F / y_cs", who);
    P4C_CHECK_ARG(rows_dtype(dy_dtype), "%s: bad dtype %d", who, dy_dtype);
    P4C_CHECK_ARG(!g_next2 || (dy_dtype == g2_dtype && g2_cs >= F), "%s: g_next2 must have the dtype of dy and g2_cs >= F", who);
    const int64_t NP = (int64_t)Hp * Wp;
    hipStream_t st = as_stream(stream);
    // the network rows in quads: whole quads per row, 16-byte aligned bases; the state side in 16-byte pieces too where F allows it
    if (!(y_cs % 4 == 0 && (!g_next2 || g2_cs % 4 == 0) && aligned16(g_next2) && aligned16(dy)))
        return fail(P4C_ERR_UNSUPPORTED, "%s: rows of dy / g_next2 must be whole quads of channels at 16-byte aligned bases", who);
    const bool state4 = F % 4 == 0 && g_next_bs % 4 == 0 && new_bs % 4 == 0 && tgt_bs % 4 == 0 && dprev_bs % 4 == 0 && aligned16(g_next) &&
                        aligned16(new_state) && aligned16(target) && aligned16(dprev) && aligned16(weights) && aligned16(std);
    const int FP4 = pow2_ge64(y_cs / 4);
    const dim3 grid(blocks_per_sample(NP, 64 / FP4, B), B);
#define P4C_WIN_BWD4(TY, ALIGNED)                                                                                                        \
    hipLaunchKernelGGL((step_bwd_win_v4_kernel<TY, ALIGNED>), grid, dim3(256), 0, st, g_next, g_next_bs, (const TY*)g_next2, g2_cs, gloss,   \
                       gloss_stride, new_state, new_bs, target, tgt_bs, std, interior_mask, force_border, weights, num_interior,         \
                       masked_count, kind, mask_mode, (TY*)dy, y_cs, dprev, dprev_bs, F, keep_prev, FP4, g)
    if (dy_dtype == P4C_F32) { if (state4) P4C_WIN_BWD4(float, true); else P4C_WIN_BWD4(float, false); }
    else { if (state4) P4C_WIN_BWD4(bf16, true); else P4C_WIN_BWD4(bf16, false); }
#undef P4C_WIN_BWD4
    P4C_CHECK_LAUNCH(who);
    return P4C_OK;
}
