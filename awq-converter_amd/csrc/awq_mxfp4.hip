// awq_mxfp4.hip — OCP microscaling FP4 (MXFP4) weights (include/awq_hip.h awq_quantize_mxfp4,
// awq_dequantize_mxfp4, awq_mxfp4_error).  Self-contained: the three entry points,
// their validation and kernels.
//
// The format.  A weight [rows, K], K % 32 == 0, is a flat run of blocks of 32 consecutive elements
// (a block never leaves its row, so the rows do not matter to the kernels: element i is in block
// i / 32, code byte i / 2, dword i / 8).  A block has one scale byte e (E8M0: 2^(e - 127), 255 =
// NaN) and 32 four-bit codes (E2M1: bit 3 the sign, bits 2..0 the magnitudes 0, 0.5, 1, 1.5, 2, 3,
// 4, 6), element 2j in the low nibble of byte j.
//
// The scale.  With E the biased fp32 exponent of amax = max |x| over the block (0 for an fp32
// subnormal), floor(log2 amax) - 2 clamped to [-127, 127] plus 127 is e = max(E, 2) - 2: no
// logarithm, no float compare; amax == 0 gives 127.  "ceil" adds one when amax 2^-X > 6 (no element
// saturates), "mse" when the block's squared error with X + 1 is strictly smaller.  Neither e + 1
// ever passes 253.  A block holding a NaN or an inf gets e = 255 and zero codes.
//
// The element.  v = |x| 2^-X is exact (a power-of-two product; where it is subnormal it rounds to
// code 0 either way), saturated at 6.  E2M1 is a float with one mantissa bit, so rounding to nearest,
// ties to the even code, is ONE fp32 addition of 2^(22 + k), k = max(exponent of v, 0): the sum's ulp
// is the grid's step at v (0.5 below 2, 1 below 4, 2 above) and the adder's own round-to-nearest-even
// does the rounding; the code is the sum's low mantissa bits plus 2 k.  The sum minus the constant is
// the rounded magnitude, which the "mse" rule's error uses.  fp32 subnormals are kept (the default of
// the gfx950 build): a block whose amax is below 2^-125 multiplies them by 2^127.
//
// The "mse" sums are taken in the scaled domain of X: sum (v - m0)^2 against 4 sum (v / 2 - m1)^2, the
// two errors divided by 4^X — exact scalings, so the comparison is the definition's, and no square
// underflows for small weights.  fp32, a lane's 8 elements in order from +0, then the quad's tree
// (awq_lanes.h: own + lane ^ 1, then + lane ^ 2).
#include <algorithm>

#include "awq_mxfp4.h"

namespace awq {
namespace {

constexpr unsigned kDequantBlocks = 256 * 16;

// ---------------------------------------------------------------------------------------
// Quantize.  One wave per trip over a 2048-element segment (awq_internal.h's tile: 4 KiB of 16-bit
// input), a capped grid striding over the segments.  Load j of 4 covers the segment's elements
// [512 j, 512 (j + 1)): lane l its 8 elements at 8 l, one 16-B nt load (two for fp32), so a block is
// the quad l / 4 and every reduction is two DPP quad steps.  A lane stores its 8 codes as one dword
// (256 contiguous bytes per wave and load).  The 16 scale bytes of a load are gathered over each
// 16-lane row (byte position = the quad's place in the row, or-ed over the row's two mirrors) into one
// dword per row; lane j of a row keeps load j's, and after the four loads lanes 0..3 of every row
// store the segment's 16 scale dwords in one instruction.  The last segment of a tensor may be short
// (any multiple of 32 elements): its loads and code stores are cut by the buffer range, its scale
// bytes are stored one by one.
// ---------------------------------------------------------------------------------------
template <typename F, int RULE>
__global__ __launch_bounds__(64) void mxfp4_quant_kernel(const void* __restrict__ x, uint8_t* __restrict__ codes,
                                                         uint8_t* __restrict__ scales, int64_t n_elems,
                                                         int64_t tiles) {
    const int lane = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t e0 = tile * kTileElems;
        const uint32_t te = (uint32_t)min((int64_t)kTileElems, n_elems - e0);   // elements of this segment
        const __amdgpu_buffer_rsrc_t rx = rsrc((const char*)x + e0 * F::kBytes, te * (uint32_t)F::kBytes);
        const __amdgpu_buffer_rsrc_t rc = rsrc(codes + e0 / 2, te / 2u);
        Chunk<F::NW> v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int h = 0; h < F::NW; ++h)
                v[j].w[h] = __builtin_amdgcn_raw_buffer_load_b128(
                    rx, (uint32_t)(j * 512 * F::kBytes + lane * 8 * F::kBytes + 16 * h), 0, AWQ_LOAD_AUX);

        uint32_t eb[4], sd = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t word;
            eb[j] = mxfp4_block<F, RULE>(v[j], word);
            __builtin_amdgcn_raw_buffer_store_b32(word, rc, (uint32_t)(j * 256 + lane * 4), 0, AWQ_STORE_AUX);
            gather_scale_bytes(eb[j], lane, j, sd);
        }
        store_scale_bytes(scales + e0 / kBlockElems, te, lane, sd, eb);
    }
}

// ---------------------------------------------------------------------------------------
// The value of a code at a scale byte: +-mag 2^(e - 127) as fp32.  The magnitude's fp32 bits are the
// code itself above exponent 126 (codes 2..7: exponent code / 2 - 1, mantissa bit code & 1); codes 0
// and 1 are 0 and 0.5.  The product with the scale is exact (two significant bits) down to 2^-128,
// a subnormal the build keeps, and overflows to inf above fp32's range.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float fp4_value(uint32_t code, float scale) {
    const uint32_t c = code & 7u;
    const uint32_t mag = c >= 2u ? (c << 22) + 0x3F000000u : c * 0x3F000000u;
    return __uint_as_float(mag | ((code & 8u) << 28)) * scale;
}

// Dequantize: a lane per dword of codes (8 elements) plus its block's scale byte, one or two 16-B
// stores; a capped grid striding over the dwords.  One rounding into the output type: the fp32
// product is exact, bf16 keeps its upper half exactly, fp16 is the hardware's RNE conversion.
template <int OD>
__global__ __launch_bounds__(256) void mxfp4_dequant_kernel(const uint32_t* __restrict__ codes,
                                                            const uint8_t* __restrict__ scales, int64_t n_words,
                                                            void* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * 256) {
        const uint32_t w = __builtin_nontemporal_load(codes + i);
        const uint32_t e = scales[i >> 2];
        const float scale = fp4_scale(e);
        uint32_t f[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            f[k] = e == 255u ? 0x7FC00000u : __float_as_uint(fp4_value(w >> (4 * k), scale));
        if (OD == AWQ_DTYPE_F32) {
            u4* o = (u4*)out + 2 * i;
            __builtin_nontemporal_store((u4){f[0], f[1], f[2], f[3]}, o);
            __builtin_nontemporal_store((u4){f[4], f[5], f[6], f[7]}, o + 1);
        } else {
            uint32_t h[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (OD == AWQ_DTYPE_BF16) {
                    h[k] = (f[2 * k] >> 16) | (f[2 * k + 1] & 0xFFFF0000u);
                } else {
                    // the magnitude converted, the sign bit copied: the conversion gives an fp32
                    // subnormal (a value below 2^-126, zero in fp16) the sign +
                    const uint16_t lo = __builtin_bit_cast(uint16_t, (_Float16)__uint_as_float(f[2 * k] & 0x7FFFFFFFu));
                    const uint16_t hi = __builtin_bit_cast(uint16_t, (_Float16)__uint_as_float(f[2 * k + 1] & 0x7FFFFFFFu));
                    h[k] = (uint32_t)lo | ((uint32_t)hi << 16) | ((f[2 * k] >> 16) & 0x8000u) | (f[2 * k + 1] & 0x80000000u);
                }
            }
            __builtin_nontemporal_store((u4){h[0], h[1], h[2], h[3]}, (u4*)out + i);
        }
    }
}

// ---------------------------------------------------------------------------------------
// The error report's level 1, awq_quant_error's streaming kernel at group_size 32 with this format's
// value in place of the integer one: one wave per 2048-element segment = 64 blocks, load j of 4 the
// elements [512 j, 512 (j + 1)), lane l its 8 elements plus their dword of codes.  Lane l also owns
// ONE block of the segment, slot (l & 3) * 16 + l / 4: it loads that block's scale byte, hands it to
// the block's quad for load j by a quad broadcast of lane j's value, and stores the block's figures.
// Per block: ErrAcc over a lane's 8 elements in order, then the quad's tree (awq_lanes.h).
// ---------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(64) void mxfp4_error_kernel(const void* __restrict__ x,
                                                         const uint32_t* __restrict__ codes,
                                                         const uint8_t* __restrict__ scales, int64_t n_elems,
                                                         int64_t n_blocks, int64_t tiles, float* __restrict__ stats,
                                                         int32_t* __restrict__ nonfinite) {
    constexpr int S = kTileElems / kBlockElems;   // 64 block slots per segment
    const int lane = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t e0 = tile * kTileElems;
        const uint32_t te = (uint32_t)min((int64_t)kTileElems, n_elems - e0);
        const __amdgpu_buffer_rsrc_t rx = rsrc((const char*)x + e0 * F::kBytes, te * (uint32_t)F::kBytes);
        const __amdgpu_buffer_rsrc_t rc = rsrc((const char*)codes + e0 / 2, te / 2u);
        Chunk<F::NW> v[4];
        uint32_t cw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int h = 0; h < F::NW; ++h)
                v[j].w[h] = __builtin_amdgcn_raw_buffer_load_b128(
                    rx, (uint32_t)(j * 512 * F::kBytes + lane * 8 * F::kBytes + 16 * h), 0, AWQ_LOAD_AUX);
            cw[j] = __builtin_amdgcn_raw_buffer_load_b32(rc, (uint32_t)(j * 256 + lane * 4), 0, AWQ_LOAD_AUX);
        }
        const uint32_t pslot = (uint32_t)(lane & 3) * (S / 4) + (uint32_t)lane / 4u;
        const bool powner = pslot < te / kBlockElems;
        const int64_t pb = tile * S + pslot;
        const uint32_t sbyte = powner ? scales[pb] : 127u;

        float oa = 0.0f, oe = 0.0f, op = 0.0f;
        uint32_t om = 0;
        int ob = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t e = bcast_u(j, sbyte);
            // e = 255: inf, so every product is inf or NaN and the block's 32 elements count as non-finite
            const float scale = fp4_scale(e);
            ErrAcc c;
#pragma unroll
            for (int i = 0; i < 8; ++i) c.add_dq(F::elem(v[j], i), fp4_value(cw[j] >> (4 * i), scale));
            const float ga = grp_sum<4>(c.a), ge = grp_sum<4>(c.e), gp = grp_sum<4>(c.p);
            const uint32_t gm = grp_max<4, uint32_t>(__float_as_uint(c.m));   // non-negative: bit order
            const int gb = grp_sum<4>(c.bad);
            if ((lane & 3) == j) { oa = ga; oe = ge; op = gp; om = gm; ob = gb; }
        }
        if (powner) {
            stats[pb] = oa;
            stats[n_blocks + pb] = oe;
            stats[2 * n_blocks + pb] = op;
            stats[3 * n_blocks + pb] = __uint_as_float(om);
            nonfinite[pb] = ob;
        }
    }
}

template <typename F>
void launch_quant(int rule, unsigned grid, hipStream_t st, const void* x, uint8_t* codes, uint8_t* scales, int64_t n,
                  int64_t tiles) {
#define AWQ_MX(R) \
    hipLaunchKernelGGL((mxfp4_quant_kernel<F, R>), dim3(grid), dim3(64), 0, st, x, codes, scales, n, tiles)
    if (rule == AWQ_MXFP4_FLOOR) AWQ_MX(AWQ_MXFP4_FLOOR);
    else if (rule == AWQ_MXFP4_CEIL) AWQ_MX(AWQ_MXFP4_CEIL);
    else AWQ_MX(AWQ_MXFP4_MSE);
#undef AWQ_MX
}

// out of awq_mxfp4_error: totals [5] (padded to 8 doubles), the level-2 workspace, the per-block figures
struct ErrorLayout {
    int64_t nblk, work, stats, bad, bytes;   // byte offsets
};
bool error_layout(int64_t n_blocks, ErrorLayout& l) {
    if (n_blocks >= (int64_t)0x7FFFFFFF) return false;
    l.nblk = qerror_level2_blocks(n_blocks);
    if (l.nblk < 0) return false;
    l.work = 64;
    l.stats = l.work + 40 * std::max<int64_t>(l.nblk, 1);
    l.bad = l.stats + 16 * n_blocks;
    l.bytes = l.bad + 4 * n_blocks;
    return true;
}

}  // namespace
}  // namespace awq

using namespace awq;

extern "C" int awq_quantize_mxfp4(const void* x, int dtype, int64_t rows, int64_t K, int rule, uint8_t* codes,
                                  uint8_t* scales, void* stream) {
    if (int rc = check_common("awq_quantize_mxfp4", dtype, rows, K)) return rc;
    if (!mxfp4_rule_ok(rule))
        return fail(AWQ_EINVAL, "awq_quantize_mxfp4: scale rule %d is not floor (0), ceil (1) or mse (2)", rule);
    const int64_t n = rows * K;
    if (n == 0) return AWQ_OK;
    if (!x || !codes || !scales) return fail(AWQ_EINVAL, "awq_quantize_mxfp4: null argument");
    if (!aligned(x, 16) || !aligned(codes, 4) || !aligned(scales, 4))
        return fail(AWQ_EINVAL, "awq_quantize_mxfp4: x needs 16-B alignment, codes and scales 4-B");
    hipStream_t st = (hipStream_t)stream;
    const int64_t tiles = (n + kTileElems - 1) / kTileElems;
    const unsigned grid = diag_cap((unsigned)std::min<int64_t>(tiles, kQuantWaves));
    if (dtype == AWQ_DTYPE_BF16) launch_quant<FmtBF16>(rule, grid, st, x, codes, scales, n, tiles);
    else if (dtype == AWQ_DTYPE_F16) launch_quant<FmtF16>(rule, grid, st, x, codes, scales, n, tiles);
    else launch_quant<FmtF32>(rule, grid, st, x, codes, scales, n, tiles);
    return hip_status(hipPeekAtLastError(), "awq mxfp4 quantize kernel");
}

extern "C" int awq_dequantize_mxfp4(const uint8_t* codes, const uint8_t* scales, int64_t rows, int64_t K,
                                    int out_dtype, void* out, void* stream) {
    if (int rc = check_common("awq_dequantize_mxfp4", out_dtype, rows, K)) return rc;
    const int64_t n = rows * K;
    if (n == 0) return AWQ_OK;
    if (!codes || !scales || !out) return fail(AWQ_EINVAL, "awq_dequantize_mxfp4: null argument");
    if (!aligned(codes, 4) || !aligned(out, 16))
        return fail(AWQ_EINVAL, "awq_dequantize_mxfp4: codes need 4-B alignment, out 16-B");
    hipStream_t st = (hipStream_t)stream;
    const int64_t words = n / 8;
    const unsigned grid = diag_cap((unsigned)std::min<int64_t>((words + 255) / 256, kDequantBlocks));
#define AWQ_MX(OD) \
    hipLaunchKernelGGL((mxfp4_dequant_kernel<OD>), dim3(grid), dim3(256), 0, st, (const uint32_t*)codes, scales, words, out)
    if (out_dtype == AWQ_DTYPE_BF16) AWQ_MX(AWQ_DTYPE_BF16);
    else if (out_dtype == AWQ_DTYPE_F16) AWQ_MX(AWQ_DTYPE_F16);
    else AWQ_MX(AWQ_DTYPE_F32);
#undef AWQ_MX
    return hip_status(hipPeekAtLastError(), "awq mxfp4 dequantize kernel");
}

extern "C" int64_t awq_mxfp4_error_out_bytes(int64_t rows, int64_t K) {
    ErrorLayout l;
    if (rows < 0 || K < 0 || K % kBlockElems != 0 || (rows > 0 && K > ((int64_t)1 << 60) / rows) ||
        !error_layout(rows * K / kBlockElems, l))
        return -1;
    return l.bytes;
}

extern "C" int awq_mxfp4_error(const void* x, int dtype, const uint8_t* codes, const uint8_t* scales, int64_t rows,
                               int64_t K, void* out, void* stream) {
    if (int rc = check_common("awq_mxfp4_error", dtype, rows, K)) return rc;
    const int64_t n = rows * K, nb = n / kBlockElems;
    ErrorLayout l;
    if (!error_layout(nb, l))
        return fail(AWQ_EUNSUPPORTED, "awq_mxfp4_error: %lld blocks exceed the level-2 reduce's range", (long long)nb);
    if (!out || (n > 0 && (!x || !codes || !scales))) return fail(AWQ_EINVAL, "awq_mxfp4_error: null argument");
    if (!aligned(x, 16) || !aligned(codes, 4) || !aligned(out, 8))
        return fail(AWQ_EINVAL, "awq_mxfp4_error: x needs 16-B alignment, codes 4-B, out 8-B");
    hipStream_t st = (hipStream_t)stream;
    double* totals = (double*)out;
    if (n == 0) {
        const hipError_t e = hipMemsetAsync(totals, 0, 5 * sizeof(double), st);
        return e == hipSuccess ? AWQ_OK : set_error(AWQ_EHIP, hipGetErrorString(e));
    }
    float* stats = (float*)((char*)out + l.stats);
    int32_t* bad = (int32_t*)((char*)out + l.bad);
    const int64_t tiles = (n + kTileElems - 1) / kTileElems;
    const unsigned grid = diag_cap((unsigned)std::min<int64_t>(tiles, kQuantWaves));
#define AWQ_MX(F) \
    hipLaunchKernelGGL((mxfp4_error_kernel<F>), dim3(grid), dim3(64), 0, st, x, (const uint32_t*)codes, scales, n, nb, \
                       tiles, stats, bad)
    if (dtype == AWQ_DTYPE_BF16) AWQ_MX(FmtBF16);
    else if (dtype == AWQ_DTYPE_F16) AWQ_MX(FmtF16);
    else AWQ_MX(FmtF32);
#undef AWQ_MX
    hipError_t e = hipPeekAtLastError();
    if (e == hipSuccess) e = launch_qerror_totals(stats, bad, nb, (double*)((char*)out + l.work), totals, st);
    return hip_status(e, "awq mxfp4 error kernels");
}
