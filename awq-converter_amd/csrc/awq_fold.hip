// awq_fold.hip — awq_fold_rows (include/awq_hip.h): out[r, k] = RN_D(RN_f32(fp32(w[r, k]) / row_scale[r])),
// the fold of 1 / s into the rows (or the bias, or the norm weight: K = 1) of whatever produces a
// searched linear's input.
//
// Two kernels, the same bits:
//   * streaming (w and out 16-B aligned, K % 8 == 0): the quantizer's memory structure — one wave
//     per tile of 2048 consecutive elements, 4 (fp32: 8) 16-B nt loads and stores per lane.  A
//     lane's 8-element chunk never straddles rows (K % 8 == 0), so it has ONE divisor: the row is
//     taken from the chunk's element offset, as scale_chunks (awq_fast.hip) takes the column —
//     the tile's first row and column once per wave (wave-uniform), then per chunk a compare
//     (K >= 2048: a tile touches at most two rows) or a 32-bit division (K < 2048).
//   * element (anything else): one element per lane, grid-stride.
// The division is the IEEE fp32 division (-fhip-fp32-correctly-rounded-divide-sqrt, no fast-math);
// its quotient is kept an fp32 value (opaque) and rounded once into the dtype.  Every wave loads
// its whole tile before it stores and tiles are disjoint, so out == w is safe (w and out are
// not __restrict__ for that reason).
#include <string>

#include "awq_quant.h"

namespace awq {
namespace {

template <typename F>
__device__ __forceinline__ uint32_t fold_bits(float x, float s) {
    const float y = F::rn(opaque(x / s));
    if constexpr (F::NW == 2) return __float_as_uint(y);
    else if constexpr (std::is_same<F, FmtF16>::value) return __builtin_bit_cast(uint16_t, (_Float16)y);
    else return __float_as_uint(y) >> 16;
}

template <typename F>
__global__ __launch_bounds__(64) void awq_fold_kernel(const char* w, char* out,
                                                       const float* __restrict__ row_scale, int64_t rows,
                                                       int64_t K) {
    const int lane = threadIdx.x & 63;
    const uint64_t total = (uint64_t)rows * (uint64_t)K;
    const uint64_t el0 = (uint64_t)blockIdx.x * kTileElems;   // wave-uniform
    if (el0 >= total) return;
    const uint32_t valid = (uint32_t)min((uint64_t)kTileElems, total - el0);
    const __amdgpu_buffer_rsrc_t rw = rsrc(w + el0 * F::kBytes, valid * (uint32_t)F::kBytes);
    const __amdgpu_buffer_rsrc_t ro = rsrc(out + el0 * F::kBytes, valid * (uint32_t)F::kBytes);
    Chunk<F::NW> v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < F::NW; ++h)
            v[j].w[h] = __builtin_amdgcn_raw_buffer_load_b128(
                rw, (uint32_t)(j * 512 * F::kBytes + lane * 8 * F::kBytes + 16 * h), 0, AWQ_LOAD_AUX);
    // the tile's first row and column (wave-uniform; 32-bit division where the offsets fit)
    uint64_t row0, col0;
    if (((el0 | (uint64_t)K) >> 32) == 0) {
        const uint32_t q = (uint32_t)el0 / (uint32_t)K;
        row0 = q;
        col0 = (uint32_t)el0 - q * (uint32_t)K;
    } else {
        row0 = el0 / (uint64_t)K;
        col0 = el0 - row0 * (uint64_t)K;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t in_tile = 512u * j + 8u * lane;
        const uint64_t idx = col0 + in_tile;               // < K + 2048
        uint64_t r;
        if (K >= kTileElems) r = row0 + (idx >= (uint64_t)K ? 1u : 0u);
        else r = row0 + (uint32_t)idx / (uint32_t)K;         // idx < 4096
        if (r > (uint64_t)rows - 1) r = (uint64_t)rows - 1;  // chunks past the end (loaded as zero, never stored)
        const float s = row_scale[r];
        uint32_t b[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) b[i] = fold_bits<F>(F::elem(v[j], i), s);
        if constexpr (F::NW == 2) {
            v[j].w[0] = u4{b[0], b[1], b[2], b[3]};
            v[j].w[1] = u4{b[4], b[5], b[6], b[7]};
        } else {
            v[j].w[0] = u4{b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16)};
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < F::NW; ++h)
            __builtin_amdgcn_raw_buffer_store_b128(
                v[j].w[h], ro, (uint32_t)(j * 512 * F::kBytes + lane * 8 * F::kBytes + 16 * h), 0, AWQ_STORE_AUX);
}

// any shape / alignment: one element per lane
template <typename F>
__global__ __launch_bounds__(256) void awq_fold_any_kernel(const void* w, void* out,
                                                           const float* __restrict__ row_scale, int64_t rows,
                                                           int64_t K) {
    const int64_t total = rows * K;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = K == 1 ? i : i / K;
        const float s = row_scale[r];
        if constexpr (F::NW == 2) {
            ((uint32_t*)out)[i] = fold_bits<F>(((const float*)w)[i], s);
        } else {
            ((uint16_t*)out)[i] = (uint16_t)fold_bits<F>(F::dec(((const uint16_t*)w)[i]), s);
        }
    }
}

hipError_t launch_fold_rows(const void* w, int dtype, int64_t rows, int64_t K, const float* row_scale, void* out,
                            hipStream_t stream) {
    const int64_t total = rows * K;
    if (total <= 0) return hipSuccess;
    const bool fast = K % 8 == 0 && (uintptr_t)w % 16 == 0 && (uintptr_t)out % 16 == 0;
    const int64_t tiles = (total + kTileElems - 1) / kTileElems;
    if (fast && tiles <= 0x7FFFFFFF) {
        const dim3 grid((unsigned)tiles), block(64);
        if (dtype == AWQ_DTYPE_BF16)
            hipLaunchKernelGGL(awq_fold_kernel<FmtBF16>, grid, block, 0, stream, (const char*)w, (char*)out, row_scale,
                               rows, K);
        else if (dtype == AWQ_DTYPE_F16)
            hipLaunchKernelGGL(awq_fold_kernel<FmtF16>, grid, block, 0, stream, (const char*)w, (char*)out, row_scale,
                               rows, K);
        else if (dtype == AWQ_DTYPE_F32)
            hipLaunchKernelGGL(awq_fold_kernel<FmtF32>, grid, block, 0, stream, (const char*)w, (char*)out, row_scale,
                               rows, K);
        else
            return hipErrorInvalidValue;
        return hipPeekAtLastError();
    }
    int64_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;   // grid-stride beyond
    const dim3 grid(diag_cap((unsigned)blocks)), block(256);
    if (dtype == AWQ_DTYPE_BF16)
        hipLaunchKernelGGL(awq_fold_any_kernel<FmtBF16>, grid, block, 0, stream, w, out, row_scale, rows, K);
    else if (dtype == AWQ_DTYPE_F16)
        hipLaunchKernelGGL(awq_fold_any_kernel<FmtF16>, grid, block, 0, stream, w, out, row_scale, rows, K);
    else if (dtype == AWQ_DTYPE_F32)
        hipLaunchKernelGGL(awq_fold_any_kernel<FmtF32>, grid, block, 0, stream, w, out, row_scale, rows, K);
    else
        return hipErrorInvalidValue;
    return hipPeekAtLastError();
}

}  // namespace
}  // namespace awq

// (the entry point lives here, not in awq_capi.hip: that file links without this one in the
// host-sanitizer build of the planners)
extern "C" int awq_fold_rows(const void* w, int dtype, int64_t rows, int64_t K, const float* row_scale, void* out,
                             void* stream) {
    awq::set_error(AWQ_OK, "");
    if (rows < 0 || K < 0)
        return awq::set_error(AWQ_EINVAL, ("negative shape (" + std::to_string(rows) + ", " + std::to_string(K) + ")").c_str());
    if (dtype != AWQ_DTYPE_BF16 && dtype != AWQ_DTYPE_F16 && dtype != AWQ_DTYPE_F32)
        return awq::set_error(AWQ_EUNSUPPORTED, ("scale folding takes bf16 / fp16 / fp32 tensors (dtype code " +
                                                 std::to_string(dtype) + ")").c_str());
    if (rows == 0 || K == 0) return AWQ_OK;   // empty: nothing is read, so the pointers are not looked at
    if (rows > ((int64_t)1 << 60) / K)         // rows * K (and its byte offsets) must fit int64
        return awq::set_error(AWQ_EINVAL, ("shape too large (" + std::to_string(rows) + ", " + std::to_string(K) + ")").c_str());
    if (!w || !row_scale || !out) return awq::set_error(AWQ_EINVAL, "null argument");
    return awq::hip_status(awq::launch_fold_rows(w, dtype, rows, K, row_scale, out, (hipStream_t)stream), "awq fold rows");
}
