// awq_import.hip — AutoAWQ "GEMM" layout import: the exact inverse of awq_export.hip.
//
// Input, the layout AutoAWQ's WQLinear_GEMM kernels read (K-major, packed along N with the
// interleave AWQ_ORDER: nibble i of word c holds column 8c + AWQ_ORDER[i]):
//   qweight_t int32 [K, N/8], qzeros_t int32 [G, N/8], scales_t fp16 [G, N].
// Output: this library's row-major packed layout of the [N = out_features, K = in_features]
// weight: qweight int32 [N, K/8] (nibble j of word c = element 8c+j), qzeros int32
// [N, ceil(G/8)] (the unused high fields of a row's last word are 0, as the quantize kernels
// write them), scales fp16 [N, G].  Values are unchanged.  Any output may be NULL.
//
// qweight: one workgroup per 256 (n) x 256 (k) nibble tile, the export's in-register 8 x 8
// nibble transpose between two renamings and an LDS-staged store (both HBM sides in 128-B row
// pieces); scales / qzeros: one workgroup per 64 (n) x 32 (g) tile through LDS.
#include "awq_gemm_layout.h"

namespace awq {
namespace {

// qweight grid order: n tiles fastest, the export's order — concurrent workgroups read
// neighbouring 128-B pieces of the same input rows.  Measured against k tiles fastest
// (profiles/import_bench.log, interleaved runs): 3-6 % faster (Llama-3-8B lm_head 103.7 vs
// 106.6-108.2 us, 14336 x 4096 21.0 vs 22.3 us) and meets the export's rate; the other does not.
// qweight: a lane holds the words of 8 consecutive input rows (k = 8 kb .. 8 kb + 7) at one
// input word column c (columns 8 c .. 8 c + 7 in AWQ_ORDER) and transposes the 8 x 8 nibble
// matrix in registers: word m is then output word (row 8 c + m, k-word kb).  Loads: 16 B per
// lane (8 lanes per 128-B row piece; 4-B loads when N % 32 != 0 or the pointer is not 16-B
// aligned).  The words are staged in LDS with the k-word column XOR-swizzled by c (32 distinct
// banks per 32-lane half: conflict-free writes) and stored as 16-B pieces of 128-B output rows.
__device__ __forceinline__ void untranspose_to_lds(const uint32_t (&a)[8], uint32_t (*ob)[kT2 / 8], int c, int kb) {
    uint32_t b[8];
    nibble_untranspose8(a, b);
#pragma unroll
    for (int m = 0; m < 8; ++m) ob[8 * c + m][kb ^ c] = b[m];
}
template <bool VEC, bool NT>
__global__ __launch_bounds__(256) void awq_import_qweight_kernel(const int32_t* __restrict__ qweight_t, int64_t N,
                                                                    int64_t K, int32_t* __restrict__ qweight) {
    __shared__ uint32_t ob[kT2][kT2 / 8];                 // [n in tile][output word column], swizzled
    const int64_t n0 = (int64_t)blockIdx.x * kT2, k0 = (int64_t)blockIdx.y * kT2;
    const int64_t wpr = K / 8, wpr_t = N / 8;
    const int t = threadIdx.x;
    if constexpr (VEC) {
        // N % 32 == 0, 16-B aligned rows: lanes (cq = t & 7, kb = t >> 3) read 16 B each, 8
        // lanes per 128-B row piece
        const int cq = t & 7, kb = t >> 3;
        const int64_t cg = n0 / 8 + 4 * cq;
        uint4 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int64_t k = k0 + 8 * kb + r;
            v[r] = make_uint4(0, 0, 0, 0);
            if (k < K && cg < wpr_t) {
                v[r] = *(const uint4*)(qweight_t + k * wpr_t + cg);
            }
        }
        const uint32_t a0[8] = {v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x};
        const uint32_t a1[8] = {v[0].y, v[1].y, v[2].y, v[3].y, v[4].y, v[5].y, v[6].y, v[7].y};
        const uint32_t a2[8] = {v[0].z, v[1].z, v[2].z, v[3].z, v[4].z, v[5].z, v[6].z, v[7].z};
        const uint32_t a3[8] = {v[0].w, v[1].w, v[2].w, v[3].w, v[4].w, v[5].w, v[6].w, v[7].w};
        untranspose_to_lds(a0, ob, 4 * cq + 0, kb);
        untranspose_to_lds(a1, ob, 4 * cq + 1, kb);
        untranspose_to_lds(a2, ob, 4 * cq + 2, kb);
        untranspose_to_lds(a3, ob, 4 * cq + 3, kb);
    } else {
        const int c = t & 31;
        const int64_t cg = n0 / 8 + c;                    // input word column
        uint32_t a[4][8];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int kb = (t >> 5) + 8 * m;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int64_t k = k0 + 8 * kb + r;
                a[m][r] = (k < K && cg < wpr_t) ? (uint32_t)qweight_t[k * wpr_t + cg] : 0u;
            }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) untranspose_to_lds(a[m], ob, c, (t >> 5) + 8 * m);
    }
    __syncthreads();
    // 256 n-rows x 32 words: 8 lanes per row, 4 words (16 B) each
    const int q = t & 7;
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
        const int nr = (t >> 3) + 32 * pass;
        const int64_t n = n0 + nr;
        if (n >= N) continue;
        const int sw = nr >> 3;                           // the swizzle of this row (its c)
        uint32_t w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = ob[nr][(4 * q + e) ^ sw];
        const int64_t c0 = k0 / 8 + 4 * q;                // output word column
        int32_t* dst = qweight + n * wpr + c0;
        if (c0 + 3 < wpr && ((uintptr_t)dst & 15) == 0) {
            if constexpr (NT)
                __builtin_nontemporal_store(u32x4{w[0], w[1], w[2], w[3]}, (u32x4*)dst);
            else
                *(uint4*)dst = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c0 + e < wpr) dst[e] = (int32_t)w[e];
        }
    }
}

// scales / qzeros: one 128-thread workgroup per 64 (n) x 32 (g) tile; either output may be null.
// Scales: two rows' (g even, g + 1) 16-B pieces of 8 columns per lane, paired into 32-bit words
// and staged as [n][g / 2] in LDS (column XOR-swizzled by bits 3-4 of n in whole 16-B pieces:
// 2-way writes, which cost a 4-B LDS store nothing), stored as 64-B output row pieces.  qzeros:
// the qweight tile's transpose on 32 lanes (input rows 8 gw .. 8 gw + 7 at word column c; rows
// past G read as 0, which is the padding of a row's last word), staged and stored as words.
__device__ __forceinline__ int nswz(int n) { return 4 * ((n >> 3) & 3); }
template <bool VEC>
__global__ __launch_bounds__(128) void awq_import_group_kernel(const int32_t* __restrict__ qzeros_t,
                                                               const uint16_t* __restrict__ scales_t, int64_t N,
                                                               int64_t G, int32_t* __restrict__ qzeros,
                                                               uint16_t* __restrict__ scales) {
    __shared__ __attribute__((aligned(16))) uint32_t sc[kGN][kGG / 2];   // [n][g pair], swizzled
    __shared__ uint32_t qz[kGN][kGG / 8];                 // [n][output word column]
    const int64_t n0 = (int64_t)blockIdx.x * kGN, g0 = (int64_t)blockIdx.y * kGG;
    const int64_t wpr_z = (G + 7) / 8, wpr_t = N / 8;
    const int t = threadIdx.x;
    if (scales) {
        const int nq = t & 7, p = t >> 3;                 // columns n0 + 8 nq ..; rows g0 + 2p, g0 + 2p + 1
        const int64_t n = n0 + 8 * nq, g = g0 + 2 * p;
        uint16_t lo[8], hi[8];
        if constexpr (VEC) {
            uint4 x = make_uint4(0, 0, 0, 0), y = x;
            if (n < N && g < G) x = *(const uint4*)(scales_t + g * N + n);
            if (n < N && g + 1 < G) y = *(const uint4*)(scales_t + (g + 1) * N + n);
            const uint32_t xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                lo[2 * e] = (uint16_t)xs[e]; lo[2 * e + 1] = (uint16_t)(xs[e] >> 16);
                hi[2 * e] = (uint16_t)ys[e]; hi[2 * e + 1] = (uint16_t)(ys[e] >> 16);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                lo[i] = (n < N && g < G) ? scales_t[g * N + n + i] : (uint16_t)0;
                hi[i] = (n < N && g + 1 < G) ? scales_t[(g + 1) * N + n + i] : (uint16_t)0;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int nr = 8 * nq + i;
            sc[nr][p ^ nswz(nr)] = (uint32_t)lo[i] | ((uint32_t)hi[i] << 16);
        }
    }
    if (qzeros && t < 32) {
        const int c = t >> 2, gw = t & 3;                 // columns n0 + 8c .., input rows g0 + 8 gw ..
        const int64_t cg = n0 / 8 + c;
        uint32_t a[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int64_t g = g0 + 8 * gw + r;
            a[r] = (g < G && cg < wpr_t) ? (uint32_t)qzeros_t[g * wpr_t + cg] : 0u;
        }
        uint32_t b[8];
        nibble_untranspose8(a, b);
#pragma unroll
        for (int m = 0; m < 8; ++m) qz[8 * c + m][gw] = b[m];
    }
    __syncthreads();
    // scales: 64 rows x 32 g = 4 pieces of 16 B per row, 2 per lane
    if (scales) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int idx = t + 128 * m, nr = idx >> 2, q = idx & 3;
            const int64_t n = n0 + nr, g = g0 + 8 * q;
            if (n >= N || g >= G) continue;
            const uint32_t* src = &sc[nr][(4 * q) ^ nswz(nr)];
            uint16_t* dst = scales + n * G + g;
            if constexpr (VEC) {
                *(uint4*)dst = *(const uint4*)src;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (g + 2 * e < G) dst[2 * e] = (uint16_t)src[e];
                    if (g + 2 * e + 1 < G) dst[2 * e + 1] = (uint16_t)(src[e] >> 16);
                }
            }
        }
    }
    // qzeros: 64 rows x 4 words, one word per lane and pass
    if (qzeros) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int idx = t + 128 * m, nr = idx >> 2, gw = idx & 3;
            const int64_t n = n0 + nr, w = g0 / 8 + gw;
            if (n < N && w < wpr_z) qzeros[n * wpr_z + w] = (int32_t)qz[nr][gw];
        }
    }
}

hipError_t launch_import_gemm(const int32_t* qweight_t, const int32_t* qzeros_t, const uint16_t* scales_t, int64_t N,
                              int64_t K, int64_t group_size, int32_t* qweight, int32_t* qzeros, uint16_t* scales,
                              hipStream_t stream) {
    // the export's size limit (its grid.y bound on K), and the same bound on this grid's y (N)
    if ((K + kT2 - 1) / kT2 > 65535 || (N + kT2 - 1) / kT2 > 65535) return hipErrorInvalidConfiguration;
    if (qweight) {
        // n tiles fastest: concurrent workgroups read neighbouring pieces of the same input rows
        const dim3 grid((unsigned)((N + kT2 - 1) / kT2), (unsigned)((K + kT2 - 1) / kT2));
        const bool vec = N % 32 == 0 && ((uintptr_t)qweight_t & 15) == 0;
        const bool nt = N * K / 2 >= (int64_t)AWQ_EXPORT_NT_MIN;
        auto kern = vec ? (nt ? awq_import_qweight_kernel<true, true> : awq_import_qweight_kernel<true, false>)
                        : (nt ? awq_import_qweight_kernel<false, true> : awq_import_qweight_kernel<false, false>);
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, qweight_t, N, K, qweight);
        if (hipError_t e = hipPeekAtLastError()) return e;
    }
    if (!qzeros && !scales) return hipSuccess;
    const int64_t G = K / group_size;
    const dim3 ggrid((unsigned)((N + kGN - 1) / kGN), (unsigned)((G + kGG - 1) / kGG));
    // 16-B scale accesses: whole 8-group pieces of 16-B aligned rows on both sides (N % 8 == 0)
    if (!scales || (G % 8 == 0 && ((uintptr_t)scales & 15) == 0 && ((uintptr_t)scales_t & 15) == 0))
        hipLaunchKernelGGL(awq_import_group_kernel<true>, ggrid, dim3(128), 0, stream, qzeros_t, scales_t, N, G, qzeros,
                           scales);
    else
        hipLaunchKernelGGL(awq_import_group_kernel<false>, ggrid, dim3(128), 0, stream, qzeros_t, scales_t, N, G,
                           qzeros, scales);
    return hipPeekAtLastError();
}

}  // namespace
}  // namespace awq

extern "C" int awq_import_autoawq_gemm(const int32_t* qweight_t, const int32_t* qzeros_t, const uint16_t* scales_t,
                                       int64_t N, int64_t K, int64_t group_size, int bits, int32_t* qweight,
                                       int32_t* qzeros, uint16_t* scales, void* stream) {
    using awq::fail;
    awq::set_error(AWQ_OK, "");
    // the export's refusals, word for word
    if (bits != 4) return fail(AWQ_EUNSUPPORTED, "the AutoAWQ GEMM layout is 4-bit only (bits=%d)", bits);
    if (group_size <= 0) return fail(AWQ_EINVAL, "Group size must be a positive integer: %lld", (long long)group_size);
    if (N <= 0 || K <= 0 || N % 8 != 0 || K % 8 != 0 || K % group_size != 0)
        return fail(AWQ_EINVAL, "AutoAWQ GEMM layout needs out_features %% 8 == 0 and in_features %% group_size == 0 "
                                "(N=%lld, K=%lld, group_size=%lld)", (long long)N, (long long)K, (long long)group_size);
    if (!qweight && !qzeros && !scales) return fail(AWQ_EINVAL, "null argument: at least one output is needed");
    if ((qweight && !qweight_t) || (qzeros && !qzeros_t) || (scales && !scales_t))
        return fail(AWQ_EINVAL, "null argument: an output without its input");
    return awq::hip_status(awq::launch_import_gemm(qweight_t, qzeros_t, scales_t, N, K, group_size, qweight, qzeros,
                                                   scales, (hipStream_t)stream), "awq import kernel");
}
