// awq_gptq.hip — AutoGPTQ layout (4 bits, desc_act = false) export and import of packed 4-bit
// results (include/awq_hip.h awq_export_gptq / awq_import_gptq).
//
// Row-major side, this library's packed outputs of a [N = out_features, K = in_features] weight:
//   qweight int32 [N, K/8] (nibble j of word c = field of element 8c + j), qzeros int32
//   [N, ceil(G/8)] (same packing of the zero-point fields), scales fp16 [N, G], G = K / group_size.
// GPTQ side: qweight_t int32 [K/8, N] (nibble i of word (r, n) = u[n, 8r + i]), qzeros_t int32
//   [G, N/8] (nibble i of word (g, c) = zs[g, 8c + i]), scales_t fp16 [G, N], g_idx int32 [K].
//
// A packed field is q - qmin (awq_quant.h): q itself when asymmetric, q + 8 and zero field 8 when
// symmetric.  That is GPTQ's u and z' in both modes, so `symmetric` changes no bit here: qweight
// is a plain transpose of 32-bit words (sequential nibbles along K on both sides), scales a
// transpose of 16-bit values, and qzeros an 8 x 8 nibble transpose per word with
// zs = (z' - zero_offset) & 15 (import: z' = (zs + zero_offset) & 15; the unused high fields of a
// row's last word stay 0).
//
// Both transposes stage a 64 x 64 tile in LDS, 256 threads, both HBM sides in 256-B (words) /
// 128-B (scales) row pieces.  The tile's row stride is an odd number of dwords (65 words, 66
// halves = 33 dwords): 4-B LDS accesses bank by (address / 4) mod 32 in 32-lane groups, so a
// column read (lane = row) touches 32 distinct banks.  The 16-B path keeps the 4-B LDS accesses
// (a padded row is not 16-B aligned) and widens only the HBM side; its LDS accesses are 2-way
// (16 lanes of a row piece span 8 banks of stride 4, two rows per group offset by 1), which a
// 4-B LDS store absorbs and costs a 4-B load one cycle: far below the HBM time of the tile.
// Grids are one-dimensional and not capped: one workgroup per tile.
#include "awq_gemm_layout.h"

namespace awq {
namespace {

constexpr int kTW = 64;                  // transpose tile edge, in elements (words or halves)

// in [R, C] -> out [C, R], elements of 4 B.  Tile order: r tiles fastest when r_fast (the N
// side runs fastest in both directions, as the AutoAWQ pair measured best), else c tiles.
template <bool VEC>
__global__ __launch_bounds__(256) void awq_gptq_words_kernel(const uint32_t* __restrict__ in, int64_t R, int64_t C,
                                                             int64_t tr, int64_t tc, int r_fast,
                                                             uint32_t* __restrict__ out) {
    __shared__ uint32_t tile[kTW][kTW + 1];
    const int64_t b = blockIdx.x;
    const int64_t r0 = (r_fast ? b % tr : b / tc) * kTW, c0 = (r_fast ? b / tr : b % tc) * kTW;
    const int t = threadIdx.x;
    if constexpr (VEC) {
        // C % 4 == 0 and R % 4 == 0, 16-B aligned bases: 16 lanes per 256-B row piece
        const int q = t & 15;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int row = (t >> 4) + 16 * p;
            const int64_t r = r0 + row, c = c0 + 4 * q;
            if (r < R && c < C) {
                const uint4 v = *(const uint4*)(in + r * C + c);
                tile[row][4 * q + 0] = v.x; tile[row][4 * q + 1] = v.y;
                tile[row][4 * q + 2] = v.z; tile[row][4 * q + 3] = v.w;
            }
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int col = (t >> 4) + 16 * p;
            const int64_t c = c0 + col, r = r0 + 4 * q;
            if (c < C && r < R)
                *(uint4*)(out + c * R + r) = make_uint4(tile[4 * q + 0][col], tile[4 * q + 1][col],
                                                        tile[4 * q + 2][col], tile[4 * q + 3][col]);
        }
    } else {
        const int x = t & 63;
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int row = (t >> 6) + 4 * p;
            const int64_t r = r0 + row, c = c0 + x;
            if (r < R && c < C) tile[row][x] = in[r * C + c];
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int col = (t >> 6) + 4 * p;
            const int64_t c = c0 + col, r = r0 + x;
            if (c < C && r < R) out[c * R + r] = tile[x][col];
        }
    }
}

// in [R, C] -> out [C, R], elements of 2 B (the fp16 scale bits)
template <bool VEC>
__global__ __launch_bounds__(256) void awq_gptq_halves_kernel(const uint16_t* __restrict__ in, int64_t R, int64_t C,
                                                              int64_t tr, int64_t tc, int r_fast,
                                                              uint16_t* __restrict__ out) {
    __shared__ uint16_t tile[kTW][kTW + 2];
    const int64_t b = blockIdx.x;
    const int64_t r0 = (r_fast ? b % tr : b / tc) * kTW, c0 = (r_fast ? b / tr : b % tc) * kTW;
    const int t = threadIdx.x;
    if constexpr (VEC) {
        // C % 8 == 0 and R % 8 == 0, 16-B aligned bases: 8 lanes per 128-B row piece
        const int q = t & 7;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int row = (t >> 3) + 32 * p;
            const int64_t r = r0 + row, c = c0 + 8 * q;
            if (r < R && c < C) {
                const uint4 v = *(const uint4*)(in + r * C + c);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    tile[row][8 * q + 2 * e] = (uint16_t)w[e];
                    tile[row][8 * q + 2 * e + 1] = (uint16_t)(w[e] >> 16);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int col = (t >> 3) + 32 * p;
            const int64_t c = c0 + col, r = r0 + 8 * q;
            if (c < C && r < R) {
                uint32_t w[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    w[e] = (uint32_t)tile[8 * q + 2 * e][col] | ((uint32_t)tile[8 * q + 2 * e + 1][col] << 16);
                *(uint4*)(out + c * R + r) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    } else {
        const int x = t & 63;
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int row = (t >> 6) + 4 * p;
            const int64_t r = r0 + row, c = c0 + x;
            if (r < R && c < C) tile[row][x] = in[r * C + c];
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int col = (t >> 6) + 4 * p;
            const int64_t c = c0 + col, r = r0 + x;
            if (c < C && r < R) out[c * R + r] = tile[x][col];
        }
    }
}

// rows a[0..7] of 8 nibbles -> b[j] = nibble j of every row, row i at nibble i (its own inverse)
__device__ __forceinline__ void nibble_transpose8_seq(const uint32_t (&a)[8], uint32_t (&b)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) b[i] = a[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) swapn(b[i], b[i + 4], 16, 0x0000FFFFu);
#pragma unroll
    for (int i = 0; i < 8; i += 4) {
        swapn(b[i], b[i + 2], 8, 0x00FF00FFu);
        swapn(b[i + 1], b[i + 3], 8, 0x00FF00FFu);
    }
#pragma unroll
    for (int i = 0; i < 8; i += 2) swapn(b[i], b[i + 1], 4, 0x0F0F0F0Fu);
}
// every nibble of x minus / plus 1, modulo 16 (no carry between nibbles)
__device__ __forceinline__ uint32_t nibbles_dec(uint32_t x) {
    return ((x | 0x88888888u) - 0x11111111u) ^ (~x & 0x88888888u);
}
__device__ __forceinline__ uint32_t nibbles_inc(uint32_t x) {
    return ((x & 0x77777777u) + 0x11111111u) ^ (x & 0x88888888u);
}

// qzeros: a lane owns input words (rows 8c .. 8c + 7, word gw) of [N, wz] and output words
// (rows 8gw .. 8gw + 7, word c) of [G, N/8]; lanes run along c (the GPTQ side is the coalesced
// one: the row-major side's rows are wz <= a few words long, a gather whichever lane order).
// EXPORT: row-major -> GPTQ, zs = (z' - off) & 15; else GPTQ -> row-major, z' = (zs + off) & 15
// on the rows below G (rows past G are the padding fields: 0).
template <bool EXPORT>
__global__ __launch_bounds__(256) void awq_gptq_zeros_kernel(const uint32_t* __restrict__ in, int64_t N, int64_t G,
                                                             int off, uint32_t* __restrict__ out) {
    const int64_t wz = (G + 7) / 8, wn = N / 8;
    const int64_t c = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const int64_t gw = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= wn || gw >= wz) return;
    uint32_t a[8], b[8];
    if constexpr (EXPORT) {
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = in[(8 * c + i) * wz + gw];
        nibble_transpose8_seq(a, b);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t g = 8 * gw + j;
            if (g < G) out[g * wn + c] = off ? nibbles_dec(b[j]) : b[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t g = 8 * gw + j;
            const uint32_t v = g < G ? in[g * wn + c] : 0u;
            a[j] = (g < G && off) ? nibbles_inc(v) : v;
        }
        nibble_transpose8_seq(a, b);
#pragma unroll
        for (int i = 0; i < 8; ++i) out[(8 * c + i) * wz + gw] = b[i];
    }
}

__global__ __launch_bounds__(256) void awq_gptq_gidx_kernel(int64_t K, int64_t L, int32_t* __restrict__ g_idx) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < K) g_idx[k] = (int32_t)(k / L);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// in [R, C] -> out [C, R]
hipError_t launch_words(const int32_t* in, int64_t R, int64_t C, bool r_fast, int32_t* out, hipStream_t stream) {
    const int64_t tr = (R + kTW - 1) / kTW, tc = (C + kTW - 1) / kTW;
    const bool vec = R % 4 == 0 && C % 4 == 0 && al16(in) && al16(out);
    hipLaunchKernelGGL(vec ? awq_gptq_words_kernel<true> : awq_gptq_words_kernel<false>, dim3((unsigned)(tr * tc)),
                       dim3(256), 0, stream, (const uint32_t*)in, R, C, tr, tc, (int)r_fast, (uint32_t*)out);
    return hipPeekAtLastError();
}
hipError_t launch_halves(const uint16_t* in, int64_t R, int64_t C, bool r_fast, uint16_t* out, hipStream_t stream) {
    const int64_t tr = (R + kTW - 1) / kTW, tc = (C + kTW - 1) / kTW;
    const bool vec = R % 8 == 0 && C % 8 == 0 && al16(in) && al16(out);
    hipLaunchKernelGGL(vec ? awq_gptq_halves_kernel<true> : awq_gptq_halves_kernel<false>, dim3((unsigned)(tr * tc)),
                       dim3(256), 0, stream, in, R, C, tr, tc, (int)r_fast, out);
    return hipPeekAtLastError();
}
template <bool EXPORT>
hipError_t launch_zeros(const int32_t* in, int64_t N, int64_t G, int off, int32_t* out, hipStream_t stream) {
    const dim3 grid((unsigned)((N / 8 + 63) / 64), (unsigned)(((G + 7) / 8 + 3) / 4));
    hipLaunchKernelGGL(awq_gptq_zeros_kernel<EXPORT>, grid, dim3(256), 0, stream, (const uint32_t*)in, N, G, off,
                       (uint32_t*)out);
    return hipPeekAtLastError();
}

// the checks both entries share, in the order include/awq_hip.h documents; 0 = go on, 1 = return
// *rc (AWQ_OK for an empty weight)
bool gptq_refuses(int64_t N, int64_t K, int64_t group_size, int bits, int symmetric, int zero_offset, int* rc) {
    *rc = AWQ_OK;
    if (N < 0 || K < 0) {
        *rc = fail(AWQ_EINVAL, "negative size (N=%lld, K=%lld)", (long long)N, (long long)K);
    } else if (bits != 4) {
        *rc = fail(AWQ_EUNSUPPORTED, "the GPTQ layout is 4-bit only here (bits=%d)", bits);
    } else if (group_size <= 0) {
        *rc = fail(AWQ_EINVAL, "Group size must be a positive integer: %lld", (long long)group_size);
    } else if (N % 8 != 0 || K % 8 != 0 || K % group_size != 0) {
        *rc = fail(AWQ_EINVAL, "GPTQ layout needs out_features %% 8 == 0, in_features %% 8 == 0 and in_features %% "
                               "group_size == 0 (N=%lld, K=%lld, group_size=%lld)", (long long)N, (long long)K,
                   (long long)group_size);
    } else if (zero_offset != 0 && zero_offset != 1) {
        *rc = fail(AWQ_EINVAL, "zero_offset must be 0 (gptq_v2) or 1 (gptq): %d", zero_offset);
    } else if (symmetric != 0 && symmetric != 1) {
        *rc = fail(AWQ_EINVAL, "symmetric must be 0 or 1: %d", symmetric);
    } else if (N == 0 || K == 0) {
        return true;
    } else if ((K + kT2 - 1) / kT2 > 65535 || (N + kT2 - 1) / kT2 > 65535 || N * K > ((int64_t)1 << 42)) {
        // the AutoAWQ pair's limit on each side, and N K <= 2^42: the largest grid here, one
        // workgroup per 64 x 64 tile of a [N, K] matrix (the scales at group_size 1), stays
        // below 2^31
        *rc = fail(AWQ_EUNSUPPORTED, "GPTQ layout: N and K are limited to 65535 * 256 and N * K to 2^42 (N=%lld, "
                                     "K=%lld)", (long long)N, (long long)K);
    }
    return *rc != AWQ_OK;
}

}  // namespace
}  // namespace awq

extern "C" int awq_export_gptq(const int32_t* qweight, const int32_t* qzeros, const uint16_t* scales, int64_t N,
                               int64_t K, int64_t group_size, int bits, int symmetric, int zero_offset,
                               int32_t* qweight_t, int32_t* qzeros_t, uint16_t* scales_t, int32_t* g_idx,
                               void* stream) {
    using namespace awq;
    set_error(AWQ_OK, "");
    int rc;
    if (gptq_refuses(N, K, group_size, bits, symmetric, zero_offset, &rc)) return rc;
    if (!qweight_t && !qzeros_t && !scales_t && !g_idx)
        return fail(AWQ_EINVAL, "null argument: at least one output is needed");
    if ((qweight_t && !qweight) || (qzeros_t && !qzeros) || (scales_t && !scales))
        return fail(AWQ_EINVAL, "null argument: an output without its input");
    hipStream_t s = (hipStream_t)stream;
    const int64_t G = K / group_size;
    hipError_t e = hipSuccess;
    if (qweight_t) e = launch_words(qweight, N, K / 8, true, qweight_t, s);
    if (!e && scales_t) e = launch_halves(scales, N, G, true, scales_t, s);
    if (!e && qzeros_t) e = launch_zeros<true>(qzeros, N, G, zero_offset, qzeros_t, s);
    if (!e && g_idx) {
        hipLaunchKernelGGL(awq_gptq_gidx_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, K, group_size,
                           g_idx);
        e = hipPeekAtLastError();
    }
    return hip_status(e, "awq gptq export kernel");
}

extern "C" int awq_import_gptq(const int32_t* qweight_t, const int32_t* qzeros_t, const uint16_t* scales_t, int64_t N,
                               int64_t K, int64_t group_size, int bits, int symmetric, int zero_offset,
                               int32_t* qweight, int32_t* qzeros, uint16_t* scales, void* stream) {
    using namespace awq;
    set_error(AWQ_OK, "");
    int rc;
    if (gptq_refuses(N, K, group_size, bits, symmetric, zero_offset, &rc)) return rc;
    if (!qweight && !qzeros && !scales) return fail(AWQ_EINVAL, "null argument: at least one output is needed");
    if ((qweight && !qweight_t) || (qzeros && !qzeros_t) || (scales && !scales_t))
        return fail(AWQ_EINVAL, "null argument: an output without its input");
    hipStream_t s = (hipStream_t)stream;
    const int64_t G = K / group_size;
    hipError_t e = hipSuccess;
    if (qweight) e = launch_words(qweight_t, K / 8, N, false, qweight, s);
    if (!e && scales) e = launch_halves(scales_t, G, N, false, scales, s);
    if (!e && qzeros) e = launch_zeros<false>(qzeros_t, N, G, zero_offset, qzeros, s);
    return hip_status(e, "awq gptq import kernel");
}
