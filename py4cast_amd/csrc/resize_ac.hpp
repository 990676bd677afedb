// The element arithmetic of the align_corners = True bilinear up-sampling (csrc/resize.hip: nn.UpsamplingBilinear2d, smp's segmentation
// head), shared with the kernels that up-sample into a concatenation buffer (csrc/deeplabplus.hip): ONE statement of the source index, the
// weights, the four-pixel blend and the backward's row range, so every user computes the same function bit for bit.
#pragma once
#include "common.hpp"

namespace p4c {
namespace resize_ac {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void unpack8(u32x4 w, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[2 * j] = __builtin_bit_cast(float, w[j] << 16);
        v[2 * j + 1] = __builtin_bit_cast(float, w[j] & 0xffff0000u);
    }
}
__device__ __forceinline__ u32x4 pack8(const float (&v)[8]) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x2 p = {v[2 * j], v[2 * j + 1]};
        o[j] = __builtin_bit_cast(unsigned int, __builtin_convertvector(p, bf16x2));
    }
    return o;
}

// source coordinate o (in - 1) / (out - 1) of output index o, as torch's area_pixel_compute_scale / _source_index compute it in fp32:
// i0, i1 and the weight of i1
__device__ __forceinline__ void src_index_ac(int o, float sc, int in_size, int& i0, int& i1, float& lam) {
    const float s = sc * (float)o;
    i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    lam = s - (float)i0;
}
__host__ __device__ inline float ac_scale(int in_size, int out_size) { return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f; }

// o[0..8) = the blend of the 8-channel octets at (y0, x0), (y0, x1), (y1, x0), (y1, x1) of one sample's map xb (W columns of row stride C)
__device__ __forceinline__ void blend8(const bf16* xb, int W, int C, int y0, int y1, int x0, int x1, float ly, float lx, float (&o)[8]) {
    float a[8], bq[8], c[8], d[8];
    unpack8(*reinterpret_cast<const u32x4*>(xb + ((int64_t)y0 * W + x0) * C), a);
    unpack8(*reinterpret_cast<const u32x4*>(xb + ((int64_t)y0 * W + x1) * C), bq);
    unpack8(*reinterpret_cast<const u32x4*>(xb + ((int64_t)y1 * W + x0) * C), c);
    unpack8(*reinterpret_cast<const u32x4*>(xb + ((int64_t)y1 * W + x1) * C), d);
    const float hy0 = 1.f - ly, wx0 = 1.f - lx;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = hy0 * (wx0 * a[j] + lx * bq[j]) + ly * (wx0 * c[j] + lx * d[j]);
}

// output rows that may read input row i: s o in [i - 1, i + 1] (a conservative range; the loop checks each one exactly)
__device__ __forceinline__ void ac_range(int i, float sc, int out_size, int& lo, int& hi) {
    if (sc <= 0.f) { lo = 0; hi = out_size - 1; return; }
    lo = max(0, (int)floorf((float)(i - 1) / sc) - 1);
    hi = min(out_size - 1, (int)ceilf((float)(i + 1) / sc) + 1);
}

// acc[0..8) = the gradient of input pixel (iy, ix): the sum over the output pixels that read it of weight * dout, rows first, in
// ascending order; db = the sample's gradient map at the octet's first channel (OW columns of row stride ld)
__device__ __forceinline__ void gather8(const bf16* db, int64_t ld, int iy, int ix, int H, int W, int OH, int OW, float sy, float sx,
                                        float (&acc)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    int oy_lo, oy_hi, ox_lo, ox_hi;
    ac_range(iy, sy, OH, oy_lo, oy_hi);
    ac_range(ix, sx, OW, ox_lo, ox_hi);
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
        int y0, y1;
        float ly;
        src_index_ac(oy, sy, H, y0, y1, ly);
        const float wy = (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
        if (wy == 0.f) continue;
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            int x0, x1;
            float lx;
            src_index_ac(ox, sx, W, x0, x1, lx);
            const float w = wy * ((x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f));
            if (w == 0.f) continue;
            float g[8];
            unpack8(*reinterpret_cast<const u32x4*>(db + ((int64_t)oy * OW + ox) * ld), g);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(w, g[j], acc[j]);
        }
    }
}

}  // namespace resize_ac
}  // namespace p4c
