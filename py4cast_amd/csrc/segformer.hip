// Segformer (mfai's Segformer over lucidrains' MiT): the passes that the GEMMs of csrc/gemm.hip do not cover.  Features-last bf16
// storage, fp32 arithmetic, every sum in a fixed order (no atomics): reruns and graph replays are bit-identical.
//
//   patch gather : the overlapping patch embedding (nn.Unfold(k, stride, pad) + Conv2d(C k^2, D, 1)) and the r x r key/value reduction
//                  as ONE GEMM over gathered patch rows: cols[(b, oy, ox)][c k^2 + ky k + kx] = x[b][oy s - p + ky][ox s - p + kx][c]
//                  (zero outside) -- Unfold's own column order, so the GEMM's weight is the parameter's (D, C k^2) view.  The data
//                  gradient is the gather-form adjoint (p4c_seg_patch_scatter): every input pixel sums the columns that read it,
//                  ky then kx.
//   channel norm : lucidrains' LayerNorm over the channels, (x - mean) / (std + eps) g + b (eps on the biased standard deviation);
//                  one wave per row; the backward writes dx and per-block partials of dgamma / dbeta.
//   depthwise 3x3: groups = C, padding 1, with bias; forward, gather-form data gradient, weight / bias partials per pixel chunk.
//   SR attention : softmax(q k^T dh^-1/2) v per (sample, head) with head_dim 32 and a spatially reduced key set of up to 256 keys
//                  (masked tail), the key / value set staged once in LDS for a 64-query tile.  The forward keeps the log-sum-exp per
//                  query; the backward recomputes P per 32-key chunk and writes dK / dV partials per query tile, summed in tile order.
//   decoder sum  : out = sum_i nearest_up_{2^i}(z_i) over the four stage maps; backward: the 2^i x 2^i block sums.
//   partial sums : out (+)= sum over the blocks of a [nb][n] partial table, block order.
#include "common.hpp"

namespace p4c {
namespace seg {

typedef unsigned short u16;

__device__ __forceinline__ float bf(const bf16* p, int64_t i) { return __bfloat162float(p[i]); }

// ---------------------------------------------------------------- patch gather / scatter
__global__ void __launch_bounds__(256) patch_gather_kernel(const bf16* __restrict__ x, bf16* __restrict__ cols, int B, int H, int W, int C,
                                                           int k, int s, int pad, int Ho, int Wo) {
    const int kk = k * k, K = C * kk;
    const int64_t n = (int64_t)B * Ho * Wo * K;
    const u16* xs = reinterpret_cast<const u16*>(x);
    u16* cs = reinterpret_cast<u16*>(cols);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int col = (int)(i % K);
        const int64_t m = i / K;
        const int c = col / kk, tap = col - c * kk, ky = tap / k, kx = tap - ky * k;
        const int ox = (int)(m % Wo);
        const int64_t t = m / Wo;
        const int oy = (int)(t % Ho);
        const int64_t b = t / Ho;
        const int iy = oy * s - pad + ky, ix = ox * s - pad + kx;
        u16 v = 0;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = xs[((b * H + iy) * W + ix) * C + c];
        cs[i] = v;
    }
}

__global__ void __launch_bounds__(256) patch_scatter_kernel(const bf16* __restrict__ dcols, bf16* __restrict__ dx, int B, int H, int W, int C,
                                                            int k, int s, int pad, int Ho, int Wo, int cgrad) {
    const int kk = k * k, K = C * kk;
    const int64_t n = (int64_t)B * H * W * cgrad;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % cgrad);
        const int64_t p = i / cgrad;
        const int ix = (int)(p % W);
        const int64_t t = p / W;
        const int iy = (int)(t % H);
        const int64_t b = t / H;
        float acc = 0.f;
        for (int ky = 0; ky < k; ++ky) {
            const int ny = iy + pad - ky;
            if (ny < 0 || ny % s) continue;
            const int oy = ny / s;
            if (oy >= Ho) continue;
            for (int kx = 0; kx < k; ++kx) {
                const int nx = ix + pad - kx;
                if (nx < 0 || nx % s) continue;
                const int ox = nx / s;
                if (ox >= Wo) continue;
                acc += bf(dcols, ((b * Ho + oy) * Wo + ox) * K + c * kk + ky * k + kx);
            }
        }
        dx[p * C + c] = __float2bfloat16(acc);
    }
}

// ---------------------------------------------------------------- channel LayerNorm (std + eps)
constexpr int LN_MAXV = 8;              // channels per lane: C <= 512
constexpr int LN_ROWS_PER_BLOCK = 32;   // 4 waves x 8 rows

__global__ void __launch_bounds__(256) chan_ln_fwd_kernel(const bf16* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                          float eps, bf16* __restrict__ y, float* __restrict__ stats, int64_t R, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const bf16* xr = x + row * C;
    float v[LN_MAXV];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        const int c = lane + 64 * j;
        v[j] = c < C ? bf(xr, c) : 0.f;
        s += v[j];
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        const int c = lane + 64 * j;
        const float d = c < C ? v[j] - mean : 0.f;
        q = __builtin_fmaf(d, d, q);
    }
    const float sd = sqrtf(wave_sum(q) / (float)C);
    const float rden = 1.f / (sd + eps);
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        const int c = lane + 64 * j;
        if (c < C) y[row * C + c] = __float2bfloat16((v[j] - mean) * rden * g[c] + b[c]);
    }
    if (lane == 0) {
        stats[2 * row] = mean;
        stats[2 * row + 1] = sd;
    }
}

// dx = (1 / d) (dxh - mean(dxh) - xh (d / sd) mean(dxh xh)) (+ dadd), d = sd + eps, xh = (x - mean) / d, dxh = dy g;
// partial[blk][0][c] = sum dy xh, partial[blk][1][c] = sum dy over the block's rows (wave order, then row order)
__global__ void __launch_bounds__(256) chan_ln_bwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy, const float* __restrict__ g,
                                                          const float* __restrict__ stats, float eps, const bf16* __restrict__ dadd,
                                                          bf16* __restrict__ dx, float* __restrict__ partial, int64_t R, int C) {
    __shared__ float red[4][2][LN_MAXV * 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float sg[LN_MAXV], sb[LN_MAXV];
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) sg[j] = sb[j] = 0.f;
    for (int r = 0; r < LN_ROWS_PER_BLOCK / 4; ++r) {
        const int64_t row = (int64_t)blockIdx.x * LN_ROWS_PER_BLOCK + wv * (LN_ROWS_PER_BLOCK / 4) + r;
        if (row >= R) break;
        const float mean = stats[2 * row], sd = stats[2 * row + 1];
        const float d = sd + eps, rd = 1.f / d;
        const float ratio = sd > 0.f ? d / sd : 0.f;
        float xh[LN_MAXV], gx[LN_MAXV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < LN_MAXV; ++j) {
            const int c = lane + 64 * j;
            xh[j] = gx[j] = 0.f;
            if (c < C) {
                const float dv = bf(dy, row * C + c);
                xh[j] = (bf(x, row * C + c) - mean) * rd;
                gx[j] = dv * g[c];
                sg[j] = __builtin_fmaf(dv, xh[j], sg[j]);
                sb[j] += dv;
                s1 += gx[j];
                s2 = __builtin_fmaf(gx[j], xh[j], s2);
            }
        }
        const float m1 = wave_sum(s1) / (float)C, m2 = wave_sum(s2) / (float)C * ratio;
#pragma unroll
        for (int j = 0; j < LN_MAXV; ++j) {
            const int c = lane + 64 * j;
            if (c < C) {
                float v = (gx[j] - m1 - xh[j] * m2) * rd;
                if (dadd) v += bf(dadd, row * C + c);
                dx[row * C + c] = __float2bfloat16(v);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < LN_MAXV; ++j) {
        red[wv][0][lane + 64 * j] = sg[j];
        red[wv][1][lane + 64 * j] = sb[j];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * C; e += 256) {
        const int which = e / C, c = e - which * C;
        const float t = ((red[0][which][c] + red[1][which][c]) + red[2][which][c]) + red[3][which][c];
        partial[((int64_t)blockIdx.x * 2 + which) * C + c] = t;
    }
}

// ---------------------------------------------------------------- partial tables
__global__ void __launch_bounds__(256) reduce_partials_kernel(const float* __restrict__ partial, int nb, int n1, float* __restrict__ out1, int n2,
                                                              float* __restrict__ out2, int accumulate) {
    const int n = n1 + n2;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        float t = 0.f;
        for (int r = 0; r < nb; ++r) t += partial[(int64_t)r * n + e];
        float* o = e < n1 ? out1 + e : out2 + (e - n1);
        *o = accumulate ? *o + t : t;
    }
}

// ---------------------------------------------------------------- depthwise 3x3 (padding 1, bias)
// thread = 8 channels of one pixel; w (C, 9) fp32 (the (C, 1, 3, 3) parameter)
__device__ __forceinline__ void load8(const bf16* p, float* v) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const unsigned int a[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[2 * j] = __uint_as_float(a[j] << 16);
        v[2 * j + 1] = __uint_as_float(a[j] & 0xffff0000u);
    }
}
__device__ __forceinline__ void store8(bf16* p, const float* v) {
    bf16 o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = __float2bfloat16(v[j]);
    *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(o);
}

template <bool DGRAD>
__global__ void __launch_bounds__(256) dw3x3_kernel(const bf16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                    bf16* __restrict__ y, int B, int H, int W, int C) {
    const int cg = C >> 3;
    const int64_t n = (int64_t)B * H * W * cg;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c0 = (int)(i % cg) * 8;
        const int64_t p = i / cg;
        const int px = (int)(p % W);
        const int64_t t = p / W;
        const int py = (int)(t % H);
        const int64_t b = t / H;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = (!DGRAD && bias) ? bias[c0 + j] : 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            // forward: y[p] += w[t] x[p + off_t]; data gradient: dx[p] += w[t] dy[p - off_t]
            const int sy = DGRAD ? py - dy : py + dy, sx = DGRAD ? px - dx : px + dx;
            if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
            float v[8];
            load8(x + ((b * H + sy) * W + sx) * C + c0, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(w[(c0 + j) * 9 + tap], v[j], acc[j]);
        }
        store8(y + p * C + c0, acc);
    }
}

constexpr int DW_PIX_PER_BLOCK = 256;

// grid (blocks over pixel chunks, channel-group blocks of 64), block (64, 4): partial[(blk * 4 + ty)][10 C] = [dw (C, 9) | db (C)]
__global__ void __launch_bounds__(256) dw3x3_wgrad_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy, float* __restrict__ partial,
                                                          int B, int H, int W, int C) {
    const int cgi = blockIdx.y * 64 + threadIdx.x, ty = threadIdx.y;
    const int64_t P = (int64_t)B * H * W;
    const int64_t row = (int64_t)blockIdx.x * 4 + ty;
    if (cgi * 8 >= C) return;
    const int c0 = cgi * 8;
    float aw[9][8], ab[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        ab[j] = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) aw[t][j] = 0.f;
    }
    const int64_t p0 = (int64_t)blockIdx.x * DW_PIX_PER_BLOCK;
    for (int q = ty; q < DW_PIX_PER_BLOCK; q += 4) {
        const int64_t p = p0 + q;
        if (p >= P) break;
        const int px = (int)(p % W);
        const int64_t t = p / W;
        const int py = (int)(t % H);
        const int64_t b = t / H;
        float g[8];
        load8(dy + p * C + c0, g);
#pragma unroll
        for (int j = 0; j < 8; ++j) ab[j] += g[j];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int sy = py + tap / 3 - 1, sx = px + tap % 3 - 1;
            if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
            float v[8];
            load8(x + ((b * H + sy) * W + sx) * C + c0, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) aw[tap][j] = __builtin_fmaf(g[j], v[j], aw[tap][j]);
        }
    }
    float* out = partial + row * (int64_t)(10 * C);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int t = 0; t < 9; ++t) out[(c0 + j) * 9 + t] = aw[t][j];
        out[9 * C + c0 + j] = ab[j];
    }
}

// ---------------------------------------------------------------- spatial-reduction attention, head_dim 32
constexpr int DH = 32;
constexpr int QT = 64;      // queries per tile
constexpr int KC = 32;      // keys per backward chunk

// block = 64 threads (one query each); LDS: K, V of the (sample, head) as fp32 [Nk][32]
__global__ void __launch_bounds__(64) sra_fwd_kernel(const bf16* __restrict__ q, const bf16* __restrict__ kv, bf16* __restrict__ out,
                                                     float* __restrict__ lse, int Nq, int Nk, int heads, float scale) {
    extern __shared__ float smem[];
    float* Ks = smem;
    float* Vs = smem + Nk * DH;
    const int tile = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int D = heads * DH;
    const bf16* kvb = kv + (int64_t)b * Nk * 2 * D;
    for (int e = threadIdx.x; e < Nk * DH; e += 64) {
        const int j = e / DH, d = e - j * DH;
        Ks[e] = bf(kvb, (int64_t)j * 2 * D + h * DH + d);
        Vs[e] = bf(kvb, (int64_t)j * 2 * D + D + h * DH + d);
    }
    __syncthreads();
    const int qi = tile * QT + threadIdx.x;
    if (qi >= Nq) return;
    const int64_t qrow = ((int64_t)b * Nq + qi) * D + h * DH;
    float qv[DH];
#pragma unroll
    for (int d = 0; d < DH; d += 8) load8(q + qrow + d, qv + d);
#pragma unroll
    for (int d = 0; d < DH; ++d) qv[d] *= scale;
    float m = -INFINITY;
    for (int j = 0; j < Nk; ++j) {
        const float4* kr = reinterpret_cast<const float4*>(Ks + j * DH);
        float s = 0.f;
#pragma unroll
        for (int d4 = 0; d4 < DH / 4; ++d4) {
            const float4 kk = kr[d4];
            s = __builtin_fmaf(qv[4 * d4], kk.x, s);
            s = __builtin_fmaf(qv[4 * d4 + 1], kk.y, s);
            s = __builtin_fmaf(qv[4 * d4 + 2], kk.z, s);
            s = __builtin_fmaf(qv[4 * d4 + 3], kk.w, s);
        }
        m = fmaxf(m, s);
    }
    float o[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) o[d] = 0.f;
    float l = 0.f;
    for (int j = 0; j < Nk; ++j) {
        const float4* kr = reinterpret_cast<const float4*>(Ks + j * DH);
        float s = 0.f;
#pragma unroll
        for (int d4 = 0; d4 < DH / 4; ++d4) {
            const float4 kk = kr[d4];
            s = __builtin_fmaf(qv[4 * d4], kk.x, s);
            s = __builtin_fmaf(qv[4 * d4 + 1], kk.y, s);
            s = __builtin_fmaf(qv[4 * d4 + 2], kk.z, s);
            s = __builtin_fmaf(qv[4 * d4 + 3], kk.w, s);
        }
        const float p = __expf(s - m);
        l += p;
        const float4* vr = reinterpret_cast<const float4*>(Vs + j * DH);
#pragma unroll
        for (int d4 = 0; d4 < DH / 4; ++d4) {
            const float4 vv = vr[d4];
            o[4 * d4] = __builtin_fmaf(p, vv.x, o[4 * d4]);
            o[4 * d4 + 1] = __builtin_fmaf(p, vv.y, o[4 * d4 + 1]);
            o[4 * d4 + 2] = __builtin_fmaf(p, vv.z, o[4 * d4 + 2]);
            o[4 * d4 + 3] = __builtin_fmaf(p, vv.w, o[4 * d4 + 3]);
        }
    }
    const float rl = 1.f / l;
#pragma unroll
    for (int d = 0; d < DH; ++d) o[d] *= rl;
#pragma unroll
    for (int d = 0; d < DH; d += 8) store8(out + qrow + d, o + d);
    lse[((int64_t)b * heads + h) * Nq + qi] = m + __logf(l);
}

// block = 256 threads over one 64-query tile of one (sample, head).  dq rows like q; part[b][h][tile][Nk][64] = (dK | dV) of the tile
__global__ void __launch_bounds__(256) sra_bwd_kernel(const bf16* __restrict__ q, const bf16* __restrict__ kv, const bf16* __restrict__ out,
                                                      const bf16* __restrict__ dout, const float* __restrict__ lse, bf16* __restrict__ dq,
                                                      float* __restrict__ part, int Nq, int Nk, int heads, float scale) {
    extern __shared__ float smem[];
    // rows of 33 floats: the P / dS loop has consecutive lanes on consecutive keys at the same d (stride 32 = one LDS bank)
    float* Ks = smem;                       // [Nk][33]
    float* Vs = Ks + Nk * (DH + 1);         // [Nk][33]
    float* Qs = Vs + Nk * (DH + 1);         // [64][33] (unscaled)
    float* Gs = Qs + QT * (DH + 1);         // [64][33] dO
    float* Ps = Gs + QT * (DH + 1);         // [64][KC + 1]
    float* Ss = Ps + QT * (KC + 1);         // [64][KC + 1] dS
    float* Ls = Ss + QT * (KC + 1);         // [64] lse
    float* Dd = Ls + QT;                    // [64] rowsum(dO O)
    const int tile = blockIdx.x, h = blockIdx.y, b = blockIdx.z, ntiles = gridDim.x;
    const int D = heads * DH, tid = threadIdx.x;
    const bf16* kvb = kv + (int64_t)b * Nk * 2 * D;
    for (int e = tid; e < Nk * DH; e += 256) {
        const int j = e / DH, d = e - j * DH;
        Ks[j * (DH + 1) + d] = bf(kvb, (int64_t)j * 2 * D + h * DH + d);
        Vs[j * (DH + 1) + d] = bf(kvb, (int64_t)j * 2 * D + D + h * DH + d);
    }
    const int q0 = tile * QT;
    for (int e = tid; e < QT * DH; e += 256) {
        const int i = e / DH, d = e - i * DH;
        const int qi = q0 + i;
        float qv = 0.f, gv = 0.f;
        if (qi < Nq) {
            const int64_t r = ((int64_t)b * Nq + qi) * D + h * DH + d;
            qv = bf(q, r);
            gv = bf(dout, r);
        }
        Qs[i * (DH + 1) + d] = qv;
        Gs[i * (DH + 1) + d] = gv;
    }
    if (tid < QT) {
        const int qi = q0 + tid;
        float dsum = 0.f, lv = 0.f;
        if (qi < Nq) {
            const int64_t r = ((int64_t)b * Nq + qi) * D + h * DH;
            for (int d = 0; d < DH; ++d) dsum = __builtin_fmaf(bf(dout, r + d), bf(out, r + d), dsum);
            lv = lse[((int64_t)b * heads + h) * Nq + qi];
        }
        Ls[tid] = lv;
        Dd[tid] = dsum;
    }
    __syncthreads();
    // dQ ownership: query qi = tid / 4, dims (tid % 4) * 8 .. + 8
    const int oq = tid >> 2, od = (tid & 3) * 8;
    float dqa[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) dqa[j] = 0.f;
    float* pt = part + ((((int64_t)b * heads + h) * ntiles + tile) * Nk) * 64;
    for (int j0 = 0; j0 < Nk; j0 += KC) {
        // P and dS of the chunk: 64 x 32 entries, 8 per thread
        for (int e = tid; e < QT * KC; e += 256) {
            const int i = e / KC, jj = e - i * KC, j = j0 + jj;
            float p = 0.f, ds = 0.f;
            if (j < Nk && q0 + i < Nq) {
                float s = 0.f, dp = 0.f;
#pragma unroll
                for (int d = 0; d < DH; ++d) {
                    s = __builtin_fmaf(Qs[i * (DH + 1) + d], Ks[j * (DH + 1) + d], s);
                    dp = __builtin_fmaf(Gs[i * (DH + 1) + d], Vs[j * (DH + 1) + d], dp);
                }
                p = __expf(s * scale - Ls[i]);
                ds = p * (dp - Dd[i]);
            }
            Ps[i * (KC + 1) + jj] = p;
            Ss[i * (KC + 1) + jj] = ds;
        }
        __syncthreads();
        const int jn = Nk - j0 < KC ? Nk - j0 : KC;
        for (int jj = 0; jj < jn; ++jj) {
            const float ds = Ss[oq * (KC + 1) + jj];
#pragma unroll
            for (int j = 0; j < 8; ++j) dqa[j] = __builtin_fmaf(ds, Ks[(j0 + jj) * (DH + 1) + od + j], dqa[j]);
        }
        // dK, dV of the chunk's keys over the tile's queries (query order): 32 x 32 entries each, 4 + 4 per thread
        for (int e = tid; e < KC * DH; e += 256) {
            const int jj = e / DH, d = e - jj * DH;
            if (jj >= jn) continue;
            float dk = 0.f, dv = 0.f;
            for (int i = 0; i < QT; ++i) {
                dk = __builtin_fmaf(Ss[i * (KC + 1) + jj], Qs[i * (DH + 1) + d], dk);
                dv = __builtin_fmaf(Ps[i * (KC + 1) + jj], Gs[i * (DH + 1) + d], dv);
            }
            pt[(int64_t)(j0 + jj) * 64 + d] = dk * scale;
            pt[(int64_t)(j0 + jj) * 64 + DH + d] = dv;
        }
        __syncthreads();
    }
    const int qi = q0 + oq;
    if (qi < Nq) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = dqa[j] * scale;
        store8(dq + ((int64_t)b * Nq + qi) * D + h * DH + od, v);
    }
}

// dkv[b][j][h 32 + d] = sum_tile part[..][0..31], dkv[b][j][D + h 32 + d] = sum_tile part[..][32..63] (tile order)
__global__ void __launch_bounds__(256) sra_dkv_reduce_kernel(const float* __restrict__ part, bf16* __restrict__ dkv, int B, int Nk, int heads,
                                                             int ntiles) {
    const int D = heads * DH;
    const int64_t n = (int64_t)B * Nk * 2 * D;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int col = (int)(e % (2 * D));
        const int64_t bj = e / (2 * D);
        const int j = (int)(bj % Nk);
        const int b = (int)(bj / Nk);
        const int half = col >= D, hc = col - half * D, h = hc / DH, d = hc - h * DH;
        const float* src = part + (((int64_t)b * heads + h) * ntiles * Nk + j) * 64 + half * DH + d;
        float t = 0.f;
        for (int tl = 0; tl < ntiles; ++tl) t += src[(int64_t)tl * Nk * 64];
        dkv[e] = __float2bfloat16(t);
    }
}

// ---------------------------------------------------------------- decoder: nearest up-sampling sums
__global__ void __launch_bounds__(256) upsum_fwd_kernel(const bf16* __restrict__ z0, const bf16* __restrict__ z1, const bf16* __restrict__ z2,
                                                        const bf16* __restrict__ z3, bf16* __restrict__ out, int B, int H, int W, int C) {
    const int cg = C >> 3;
    const int64_t n = (int64_t)B * H * W * cg;
    const bf16* z[4] = {z0, z1, z2, z3};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c0 = (int)(i % cg) * 8;
        const int64_t p = i / cg;
        const int px = (int)(p % W);
        const int64_t t = p / W;
        const int py = (int)(t % H);
        const int64_t b = t / H;
        float acc[8], v[8];
        load8(z0 + p * C + c0, acc);
#pragma unroll
        for (int l = 1; l < 4; ++l) {
            const int Hl = H >> l, Wl = W >> l;
            load8(z[l] + ((b * Hl + (py >> l)) * Wl + (px >> l)) * C + c0, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += v[j];
        }
        store8(out + p * C + c0, acc);
    }
}

// blockIdx.y = level - 1: dz_l[b][Y][X] = sum over dy < 2^l, dx < 2^l (row-major) of dout[b][Y 2^l + dy][X 2^l + dx]
__global__ void __launch_bounds__(256) upsum_bwd_kernel(const bf16* __restrict__ dout, bf16* __restrict__ dz1, bf16* __restrict__ dz2,
                                                        bf16* __restrict__ dz3, int B, int H, int W, int C) {
    const int l = blockIdx.y + 1, f = 1 << l, Hl = H >> l, Wl = W >> l, cg = C >> 3;
    bf16* dz = l == 1 ? dz1 : (l == 2 ? dz2 : dz3);
    const int64_t n = (int64_t)B * Hl * Wl * cg;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c0 = (int)(i % cg) * 8;
        const int64_t p = i / cg;
        const int X = (int)(p % Wl);
        const int64_t t = p / Wl;
        const int Y = (int)(t % Hl);
        const int64_t b = t / Hl;
        float acc[8], v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        for (int dy = 0; dy < f; ++dy)
            for (int dx = 0; dx < f; ++dx) {
                load8(dout + ((b * H + Y * f + dy) * W + X * f + dx) * C + c0, v);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += v[j];
            }
        store8(dz + p * C + c0, acc);
    }
}

inline int grid_for(int64_t n) { return (int)((n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536); }

}  // namespace seg
}  // namespace p4c

using namespace p4c;

extern "C" int p4c_seg_patch_gather(const void* x, void* cols, int B, int H, int W, int C, int k, int stride, int pad, p4c_stream_t stream) {
    P4C_CHECK_ARG(x && cols, "p4c_seg_patch_gather: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && k > 0 && stride > 0 && pad >= 0 && H + 2 * pad >= k && W + 2 * pad >= k,
                  "p4c_seg_patch_gather: B=%d H=%d W=%d C=%d k=%d stride=%d pad=%d", B, H, W, C, k, stride, pad);
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    const int64_t n = (int64_t)B * Ho * Wo * C * k * k;
    hipLaunchKernelGGL(seg::patch_gather_kernel, dim3(seg::grid_for(n)), dim3(256), 0, as_stream(stream), (const bf16*)x, (bf16*)cols, B, H, W,
                       C, k, stride, pad, Ho, Wo);
    P4C_CHECK_LAUNCH("p4c_seg_patch_gather");
    return P4C_OK;
}

extern "C" int p4c_seg_patch_scatter(const void* dcols, void* dx, int B, int H, int W, int C, int k, int stride, int pad, int cgrad,
                                     p4c_stream_t stream) {
    P4C_CHECK_ARG(dcols && dx, "p4c_seg_patch_scatter: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && k > 0 && stride > 0 && pad >= 0 && H + 2 * pad >= k && W + 2 * pad >= k && cgrad > 0 &&
                  cgrad <= C, "p4c_seg_patch_scatter: B=%d H=%d W=%d C=%d k=%d stride=%d pad=%d cgrad=%d", B, H, W, C, k, stride, pad, cgrad);
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    const int64_t n = (int64_t)B * H * W * cgrad;
    hipLaunchKernelGGL(seg::patch_scatter_kernel, dim3(seg::grid_for(n)), dim3(256), 0, as_stream(stream), (const bf16*)dcols, (bf16*)dx, B, H, W,
                       C, k, stride, pad, Ho, Wo, cgrad);
    P4C_CHECK_LAUNCH("p4c_seg_patch_scatter");
    return P4C_OK;
}

extern "C" int p4c_seg_chan_ln_fwd(const void* x, const float* g, const float* b, float eps, void* y, float* stats, int64_t R, int C,
                                   p4c_stream_t stream) {
    P4C_CHECK_ARG(x && g && b && y && stats, "p4c_seg_chan_ln_fwd: NULL pointer");
    P4C_CHECK_ARG(R > 0 && C > 0 && C <= 64 * seg::LN_MAXV, "p4c_seg_chan_ln_fwd: R=%lld C=%d (C up to 512)", (long long)R, C);
    hipLaunchKernelGGL(seg::chan_ln_fwd_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, as_stream(stream), (const bf16*)x, g, b, eps, (bf16*)y,
                       stats, R, C);
    P4C_CHECK_LAUNCH("p4c_seg_chan_ln_fwd");
    return P4C_OK;
}

extern "C" int p4c_seg_chan_ln_bwd_blocks(int64_t R) { return (int)((R + seg::LN_ROWS_PER_BLOCK - 1) / seg::LN_ROWS_PER_BLOCK); }

extern "C" int p4c_seg_chan_ln_bwd(const void* x, const void* dy, const float* g, const float* stats, float eps, const void* dadd, void* dx,
                                   float* partial, int64_t R, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(x && dy && g && stats && dx && partial, "p4c_seg_chan_ln_bwd: NULL pointer");
    P4C_CHECK_ARG(R > 0 && C > 0 && C <= 64 * seg::LN_MAXV, "p4c_seg_chan_ln_bwd: R=%lld C=%d (C up to 512)", (long long)R, C);
    hipLaunchKernelGGL(seg::chan_ln_bwd_kernel, dim3(p4c_seg_chan_ln_bwd_blocks(R)), dim3(256), 0, as_stream(stream), (const bf16*)x,
                       (const bf16*)dy, g, stats, eps, (const bf16*)dadd, (bf16*)dx, partial, R, C);
    P4C_CHECK_LAUNCH("p4c_seg_chan_ln_bwd");
    return P4C_OK;
}

extern "C" int p4c_seg_reduce_partials(const float* partial, int nb, int n1, float* out1, int n2, float* out2, int accumulate,
                                       p4c_stream_t stream) {
    P4C_CHECK_ARG(partial && out1 && (n2 == 0 || out2), "p4c_seg_reduce_partials: NULL pointer");
    P4C_CHECK_ARG(nb > 0 && n1 > 0 && n2 >= 0, "p4c_seg_reduce_partials: nb=%d n1=%d n2=%d", nb, n1, n2);
    hipLaunchKernelGGL(seg::reduce_partials_kernel, dim3(seg::grid_for(n1 + n2)), dim3(256), 0, as_stream(stream), partial, nb, n1, out1, n2, out2,
                       accumulate);
    P4C_CHECK_LAUNCH("p4c_seg_reduce_partials");
    return P4C_OK;
}

extern "C" int p4c_seg_dw3x3_fwd(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(x && w && y, "p4c_seg_dw3x3_fwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "p4c_seg_dw3x3_fwd: B=%d H=%d W=%d C=%d (C a multiple of 8)", B, H, W, C);
    const int64_t n = (int64_t)B * H * W * (C / 8);
    hipLaunchKernelGGL(seg::dw3x3_kernel<false>, dim3(seg::grid_for(n)), dim3(256), 0, as_stream(stream), (const bf16*)x, w, bias, (bf16*)y, B, H,
                       W, C);
    P4C_CHECK_LAUNCH("p4c_seg_dw3x3_fwd");
    return P4C_OK;
}

extern "C" int p4c_seg_dw3x3_dgrad(const void* dy, const float* w, void* dx, int B, int H, int W, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(dy && w && dx, "p4c_seg_dw3x3_dgrad: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "p4c_seg_dw3x3_dgrad: B=%d H=%d W=%d C=%d (C a multiple of 8)", B, H, W, C);
    const int64_t n = (int64_t)B * H * W * (C / 8);
    hipLaunchKernelGGL(seg::dw3x3_kernel<true>, dim3(seg::grid_for(n)), dim3(256), 0, as_stream(stream), (const bf16*)dy, w, nullptr, (bf16*)dx,
                       B, H, W, C);
    P4C_CHECK_LAUNCH("p4c_seg_dw3x3_dgrad");
    return P4C_OK;
}

extern "C" int p4c_seg_dw3x3_wgrad_rows(int B, int H, int W) {
    const int64_t P = (int64_t)B * H * W;
    return (int)(4 * ((P + seg::DW_PIX_PER_BLOCK - 1) / seg::DW_PIX_PER_BLOCK));
}

extern "C" int p4c_seg_dw3x3_wgrad(const void* x, const void* dy, float* partial, int B, int H, int W, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(x && dy && partial, "p4c_seg_dw3x3_wgrad: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "p4c_seg_dw3x3_wgrad: B=%d H=%d W=%d C=%d (C a multiple of 8)", B, H, W, C);
    const int rows = p4c_seg_dw3x3_wgrad_rows(B, H, W);
    hipLaunchKernelGGL(seg::dw3x3_wgrad_kernel, dim3(rows / 4, (C / 8 + 63) / 64), dim3(64, 4), 0, as_stream(stream), (const bf16*)x,
                       (const bf16*)dy, partial, B, H, W, C);
    P4C_CHECK_LAUNCH("p4c_seg_dw3x3_wgrad");
    return P4C_OK;
}

static size_t sra_bwd_smem(int Nk) {
    using namespace seg;
    return sizeof(float) * ((size_t)2 * Nk * (DH + 1) + 2 * QT * (DH + 1) + 2 * QT * (KC + 1) + 2 * QT);
}

extern "C" int p4c_seg_sra_fwd(const void* q, const void* kv, void* out, float* lse, int B, int Nq, int Nk, int heads, float scale,
                               p4c_stream_t stream) {
    using namespace seg;
    P4C_CHECK_ARG(q && kv && out && lse, "p4c_seg_sra_fwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && Nq > 0 && Nk > 0 && Nk <= 256 && heads > 0 && heads <= 64,
                  "p4c_seg_sra_fwd: B=%d Nq=%d Nk=%d heads=%d (Nk up to 256)", B, Nq, Nk, heads);
    const int smem = (int)(sizeof(float) * 2 * Nk * DH);
    P4C_TRY(ensure_dyn_smem((const void*)sra_fwd_kernel, smem));
    hipLaunchKernelGGL(sra_fwd_kernel, dim3((Nq + QT - 1) / QT, heads, B), dim3(64), smem, as_stream(stream), (const bf16*)q, (const bf16*)kv,
                       (bf16*)out, lse, Nq, Nk, heads, scale);
    P4C_CHECK_LAUNCH("p4c_seg_sra_fwd");
    return P4C_OK;
}

extern "C" size_t p4c_seg_sra_bwd_workspace_bytes(int B, int Nq, int Nk, int heads) {
    return sizeof(float) * (size_t)B * heads * ((Nq + seg::QT - 1) / seg::QT) * Nk * 64;
}

extern "C" int p4c_seg_sra_bwd(const void* q, const void* kv, const void* out, const void* dout, const float* lse, void* dq, void* dkv,
                               float* workspace, int B, int Nq, int Nk, int heads, float scale, p4c_stream_t stream) {
    using namespace seg;
    P4C_CHECK_ARG(q && kv && out && dout && lse && dq && dkv && workspace, "p4c_seg_sra_bwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && Nq > 0 && Nk > 0 && Nk <= 256 && heads > 0 && heads <= 64,
                  "p4c_seg_sra_bwd: B=%d Nq=%d Nk=%d heads=%d (Nk up to 256)", B, Nq, Nk, heads);
    const int ntiles = (Nq + QT - 1) / QT;
    const int smem = (int)sra_bwd_smem(Nk);
    P4C_TRY(ensure_dyn_smem((const void*)sra_bwd_kernel, smem));
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(sra_bwd_kernel, dim3(ntiles, heads, B), dim3(256), smem, st, (const bf16*)q, (const bf16*)kv, (const bf16*)out,
                       (const bf16*)dout, lse, (bf16*)dq, workspace, Nq, Nk, heads, scale);
    P4C_CHECK_LAUNCH("p4c_seg_sra_bwd");
    const int64_t n = (int64_t)B * Nk * 2 * heads * DH;
    hipLaunchKernelGGL(sra_dkv_reduce_kernel, dim3(grid_for(n)), dim3(256), 0, st, workspace, (bf16*)dkv, B, Nk, heads, ntiles);
    P4C_CHECK_LAUNCH("p4c_seg_sra_dkv_reduce");
    return P4C_OK;
}

extern "C" int p4c_seg_upsum_fwd(const void* z0, const void* z1, const void* z2, const void* z3, void* out, int B, int H, int W, int C,
                                 p4c_stream_t stream) {
    P4C_CHECK_ARG(z0 && z1 && z2 && z3 && out, "p4c_seg_upsum_fwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && C > 0 && C % 8 == 0,
                  "p4c_seg_upsum_fwd: B=%d H=%d W=%d C=%d (H, W, C multiples of 8)", B, H, W, C);
    const int64_t n = (int64_t)B * H * W * (C / 8);
    hipLaunchKernelGGL(seg::upsum_fwd_kernel, dim3(seg::grid_for(n)), dim3(256), 0, as_stream(stream), (const bf16*)z0, (const bf16*)z1,
                       (const bf16*)z2, (const bf16*)z3, (bf16*)out, B, H, W, C);
    P4C_CHECK_LAUNCH("p4c_seg_upsum_fwd");
    return P4C_OK;
}

extern "C" int p4c_seg_upsum_bwd(const void* dout, void* dz1, void* dz2, void* dz3, int B, int H, int W, int C, p4c_stream_t stream) {
    P4C_CHECK_ARG(dout && dz1 && dz2 && dz3, "p4c_seg_upsum_bwd: NULL pointer");
    P4C_CHECK_ARG(B > 0 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && C > 0 && C % 8 == 0,
                  "p4c_seg_upsum_bwd: B=%d H=%d W=%d C=%d (H, W, C multiples of 8)", B, H, W, C);
    const int64_t n = (int64_t)B * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(seg::upsum_bwd_kernel, dim3(seg::grid_for(n), 3), dim3(256), 0, as_stream(stream), (const bf16*)dout, (bf16*)dz1, (bf16*)dz2,
                       (bf16*)dz3, B, H, W, C);
    P4C_CHECK_LAUNCH("p4c_seg_upsum_bwd");
    return P4C_OK;
}
