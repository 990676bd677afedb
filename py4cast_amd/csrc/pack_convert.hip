// Planes in the files' own number format onto the standardised features-last batch, in one pass: what the rainfall accessor
// does per plane on the host in float64 (datasets/rainfall.py:116-164: np.where(arr < 0, 0, arr) / 100 * 12, arr[::-1]) and
// Sample.get_param_tensor after it (datasets/base.py:431-453: (arr - mean) / std), fused with the features-last pack of
// p4c_pack_standardize.  The planes arrive as they lie in the files (u8, i16, u16, i32, f16, f32 or f64): no host conversion.
//
// Arithmetic, to the bit (this file is built with -ffp-contract=off; hipcc's fp32 division is correctly rounded):
//   v = (float)raw (round to nearest even), v = v < floor ? floor : v (a NaN stays), v / div, v * mul, (v - mean) / std,
//   every step rounded to fp32; a div or mul of exactly 1 is skipped (it would change nothing but -0 / NaN payloads).
//
// Layout as pack_standardize_kernel (rollout.hip): a workgroup transposes `rows` rows x F columns through an LDS tile padded to
// rows + 1, so its output is one contiguous, ordered run of rows * F floats.  A row is ((b*T + t)*H + y)*W + x.  The read side
// differs: a lane loads 16 bytes, E = 16 / sizeof(element) neighbours along W, whatever the format (vec), so a wave's load is a
// run of 1 KB for every dtype.  That needs W and the plane strides to be multiples of E (a chunk then never leaves its source
// row and stays aligned); other shapes take the same kernel with E = 1.  With few features a pass takes more rows (up to 2048),
// so that the 16-byte loads of one pass still fill the workgroup; a workgroup walks the passes grid-stride.
// The E values of a lane go to LDS at a stride of E floats between lanes: an E-way bank conflict on the E writes (16-way for
// u8).  Its cost was not measured; the transposed reads and the global writes stay conflict-free and ordered.
#include "common.hpp"

namespace p4c {

constexpr int PC_MAX_COLS = 144;
constexpr int PC_BASE_ROWS = 256;
constexpr int PC_BLOCKS_PER_CU = 8;

// rows per pass: 256 x min(8, 16 / F), at least 256.  F * (rows + 1) * 4 bytes of LDS: 8 KB .. 16 KB up to F = 16, then F KB.
__host__ __device__ constexpr int pc_rows(int F) {
    return PC_BASE_ROWS * (16 / F >= 8 ? 8 : (16 / F >= 1 ? 16 / F : 1));
}

// E neighbours of one source row: one 16-byte global load (E = 16 / sizeof(S)), or one element (E = 1)
template <typename S, int E>
struct pc_load {
    static_assert(E * sizeof(S) == 16, "a chunk is 16 bytes");
    static __device__ __forceinline__ void get(const S* p, S (&v)[E]) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(1))) const u32x4 gu32x4;
        const u32x4 u = *(gu32x4*)p;
        __builtin_memcpy(v, &u, 16);
    }
};
template <typename S>
struct pc_load<S, 1> {
    static __device__ __forceinline__ void get(const S* p, S (&v)[1]) {
        typedef __attribute__((address_space(1))) const S gS;
        v[0] = *(gS*)p;
    }
};

template <typename S, int E>
__global__ void __launch_bounds__(256)
    pack_convert_kernel(const p4c_convert_feature* __restrict__ feats, float* __restrict__ out, int64_t R, int T, int H, int W, int F,
                        int rows) {
    extern __shared__ float tile[];  // [F][rows + 1]
    const int pitch = rows + 1;
    const int chunks = rows / E;     // per feature; rows is a multiple of 256, E a divisor of 16
    const int items = F * chunks;
    const uint32_t HW = (uint32_t)H * (uint32_t)W;
    const int64_t passes = (R + rows - 1) / rows;
    for (int64_t pass = blockIdx.x; pass < passes; pass += gridDim.x) {
        const int64_t r0 = pass * rows;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int f = i / chunks, c = i - f * chunks;
            const int64_t r = r0 + (int64_t)c * E;
            // vec: R is a multiple of E (W is), so a chunk lies wholly inside or wholly past the end
            if (r < R) {
                const p4c_convert_feature d = feats[f];
                const uint32_t bt = (uint32_t)r / HW, p = (uint32_t)r - bt * HW;      // R < 2^31 is checked by the host
                const uint32_t y = p / (uint32_t)W, x = p - y * (uint32_t)W;
                const uint32_t b = bt / (uint32_t)T, t = bt - b * (uint32_t)T;
                const uint32_t ys = (d.flags & P4C_CONVERT_FLIP_ROWS) ? (uint32_t)H - 1 - y : y;
                const S* src = (const S*)d.src + (int64_t)b * d.b_stride + (int64_t)t * d.t_stride + (int64_t)ys * W + x;
                S raw[E];
                pc_load<S, E>::get(src, raw);
                float* dst = tile + d.channel * pitch + c * E;
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    float v = (float)raw[k];               // v_cvt_f32_*: exact, or round to nearest even
                    if (d.flags & P4C_CONVERT_HAS_FLOOR) v = v < d.floor ? d.floor : v;
                    if (d.div != 1.f) v = v / d.div;
                    if (d.mul != 1.f) v = v * d.mul;
                    const float e = v - d.mean;
                    dst[k] = e / d.std;
                }
            }
        }
        __syncthreads();
        const int64_t rows_here = (R - r0 < rows) ? (R - r0) : rows;
        const int64_t total = rows_here * F;
        float* dst = out + r0 * F;
        int row = threadIdx.x / F, f = threadIdx.x - row * F;
        const int drow = 256 / F, df = 256 - drow * F;
        for (int64_t j = threadIdx.x; j < total; j += 256) {
            dst[j] = tile[f * pitch + row];
            row += drow;
            f += df;
            if (f >= F) { f -= F; ++row; }
        }
        __syncthreads();   // the next pass overwrites the tile
    }
}

template <typename S>
static int launch_convert(const p4c_convert_feature* feats, float* out, int vec, int64_t R, int T, int H, int W, int F,
                          hipStream_t stream) {
    constexpr int E = 16 / (int)sizeof(S);
    const int rows = pc_rows(F);
    const size_t smem = (size_t)F * (rows + 1) * sizeof(float);
    const int max_smem = PC_MAX_COLS * (PC_BASE_ROWS + 1) * 4;
    int64_t blocks = (R + rows - 1) / rows;
    const int64_t cap = (int64_t)num_cus() * PC_BLOCKS_PER_CU;
    if (blocks > cap) blocks = cap;
    if (vec) {
        P4C_CHECK_ARG(W % E == 0, "p4c_pack_convert: vec needs W = %d to be a multiple of %d elements (16 bytes)", W, E);
        P4C_TRY(ensure_dyn_smem((const void*)pack_convert_kernel<S, E>, max_smem));
        hipLaunchKernelGGL((pack_convert_kernel<S, E>), dim3((unsigned)blocks), dim3(256), smem, stream, feats, out, R, T, H, W, F, rows);
    } else {
        P4C_TRY(ensure_dyn_smem((const void*)pack_convert_kernel<S, 1>, max_smem));
        hipLaunchKernelGGL((pack_convert_kernel<S, 1>), dim3((unsigned)blocks), dim3(256), smem, stream, feats, out, R, T, H, W, F, rows);
    }
    P4C_CHECK_LAUNCH("p4c_pack_convert");
    return P4C_OK;
}

}  // namespace p4c

using namespace p4c;

extern "C" int p4c_pack_convert_rows(int F) { return (F >= 1 && F <= PC_MAX_COLS) ? pc_rows(F) : 0; }
extern "C" int p4c_pack_convert_max_blocks(void) { return num_cus() * PC_BLOCKS_PER_CU; }

extern "C" int p4c_pack_convert(const p4c_convert_feature* feats, float* out, int dtype, int vec, int B, int T, int H, int W, int F,
                                p4c_stream_t stream) {
    static_assert(sizeof(p4c_convert_feature) == 56, "descriptor layout is part of the ABI");
    P4C_CHECK_ARG(F >= 1 && F <= PC_MAX_COLS, "p4c_pack_convert: %d features: at most %d per call (LDS tile)", F, PC_MAX_COLS);
    P4C_CHECK_ARG(feats && out, "p4c_pack_convert: null pointer");
    P4C_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0, "p4c_pack_convert: bad dims (B=%d T=%d H=%d W=%d)", B, T, H, W);
    const int64_t rows = (int64_t)B * T * H * W;
    P4C_CHECK_ARG(rows < ((int64_t)1 << 31), "p4c_pack_convert: %lld rows: at most 2^31 - 1 per call", (long long)rows);
    hipStream_t s = as_stream(stream);
    switch (dtype) {
        case P4C_SRC_U8: return launch_convert<uint8_t>(feats, out, vec, rows, T, H, W, F, s);
        case P4C_SRC_I16: return launch_convert<int16_t>(feats, out, vec, rows, T, H, W, F, s);
        case P4C_SRC_U16: return launch_convert<uint16_t>(feats, out, vec, rows, T, H, W, F, s);
        case P4C_SRC_I32: return launch_convert<int32_t>(feats, out, vec, rows, T, H, W, F, s);
        case P4C_SRC_F16: return launch_convert<_Float16>(feats, out, vec, rows, T, H, W, F, s);
        case P4C_SRC_F32: return launch_convert<float>(feats, out, vec, rows, T, H, W, F, s);
        case P4C_SRC_F64: return launch_convert<double>(feats, out, vec, rows, T, H, W, F, s);
        default: break;
    }
    return ::p4c::fail(P4C_ERR_INVALID, "p4c_pack_convert: dtype %d is none of P4C_SRC_*", dtype);
}
