// awq_gptq_actorder.hip — GPTQ act-order (desc_act = true): the data path for 4-bit fields whose
// group is g_idx[k], not k / group_size (include/awq_hip.h awq_gptq_permute_rows /
// awq_gptq_gidx_from_perm / awq_gptq_check_index / awq_dequantize_gptq).
//
// GPTQ side of a [N = out_features, K = in_features] linear: qweight_t int32 [K/8, N] (nibble i of
// word (r, n) = u[n, 8r + i]), qzeros_t int32 [G, N/8], scales_t fp16 [G, N], g_idx int32 [K].  An
// input column k is a nibble plane of word row k / 8, contiguous along N: a permutation of the
// columns is a gather of nibble ROWS, and every HBM access of it is a row piece along N.
//
// Gather.  One workgroup (256 threads) owns 64 output word rows of a strip of 64 words (256 B)
// along N.  Each output word reads eight source words of its own column, so a strip of all K/8
// output rows reads its K/8 x 256 B source slice eight times over.  The workgroups of one strip
// are consecutive on ONE XCD (workgroups are dealt round-robin over the 8 XCDs: b % 8 picks the
// XCD, so strip = 8 (b / 8 / C) + b % 8 for C row chunks per strip), which keeps the slice (0.5 MB
// at K = 14336) in that XCD's L2 while the strip is live; 16-B path: 16 lanes per 256-B row piece,
// 16 rows per pass; element path: 64 lanes per row piece, 4 rows per pass.  No LDS: the nibbles
// of a word are assembled in registers.
//
// Dequantize.  One workgroup per tile of 128 k x 64 n.  Wave w reads word rows 4w .. 4w + 3 of the
// tile (64 lanes = 64 words = one 256-B row piece each), so its 32 columns are consecutive; the
// group of a column is wave-uniform (a scalar), and a word row whose eight columns stay in the
// wave's current group reuses its scale and zero (the trivial g_idx fetches them once per wave and
// tile), while any other row fetches its eight scale row pieces (128 B) and zero row pieces (32 B)
// together.  The fp16 results go through LDS as [64 n][65 dwords]: a lane stores its word's eight
// halves as four dwords at row n (bank = (n + const) mod 32: conflict-free), and the store phase
// reads a row per wave instruction, lane l dword l (consecutive banks), so out[n, k0 ..] leaves in
// 256-B (fp16 / bf16) or 512-B (fp32) row pieces along K.
#include "awq_gemm_layout.h"

namespace awq {
namespace {

constexpr int kStripW = 64;              // gather: words of a strip along N
constexpr int kStripR = 64;              // gather: output word rows per workgroup
constexpr int kDK = 128, kDN = 64;       // dequantize tile: columns (k) x rows (n)
constexpr int kDStride = kDK / 2 + 1;    // dwords per LDS row: odd

// src[8r + i] for i < 8, an entry outside [0, K) replaced by 0
__device__ __forceinline__ void load_src8(const int32_t* __restrict__ src, int64_t r, uint32_t K, uint32_t (&s)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t v = (uint32_t)src[8 * r + i];
        s[i] = v < K ? v : 0u;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void awq_gptq_permute_kernel(const uint32_t* __restrict__ in,
                                                               const int32_t* __restrict__ src, int64_t N, int64_t R,
                                                               int64_t strips, int64_t chunks,
                                                               uint32_t* __restrict__ out) {
    const int64_t b = blockIdx.x, i8 = b / 8;
    const int64_t strip = (i8 / chunks) * 8 + b % 8, chunk = i8 % chunks;
    if (strip >= strips) return;
    const int64_t c0 = strip * kStripW, r0 = chunk * kStripR;
    const uint32_t K = (uint32_t)(8 * R);
    const int t = threadIdx.x;
    if constexpr (VEC) {
        const int64_t c = c0 + 4 * (t & 15);
        if (c >= N) return;                               // (N % 4 == 0: a quad is wholly inside or outside)
#pragma unroll
        for (int p = 0; p < kStripR / 16; ++p) {
            const int64_t r = r0 + (t >> 4) + 16 * p;
            if (r >= R) break;
            uint32_t s[8];
            load_src8(src, r, K, s);
            u32x4 w[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = *(const u32x4*)(in + (int64_t)(s[i] >> 3) * N + c);
            u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; ++i) o |= ((w[i] >> (4u * (s[i] & 7u))) & 15u) << (4u * i);
            *(u32x4*)(out + r * N + c) = o;
        }
    } else {
        const int64_t c = c0 + (t & 63);
        if (c >= N) return;
#pragma unroll 4
        for (int p = 0; p < kStripR / 4; ++p) {
            const int64_t r = r0 + (t >> 6) + 4 * p;
            if (r >= R) break;
            uint32_t s[8];
            load_src8(src, r, K, s);
            uint32_t w[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = in[(int64_t)(s[i] >> 3) * N + c];
            uint32_t o = 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) o |= ((w[i] >> (4u * (s[i] & 7u))) & 15u) << (4u * i);
            out[r * N + c] = o;
        }
    }
}

__global__ __launch_bounds__(256) void awq_gptq_gidx_perm_kernel(const int32_t* __restrict__ perm, int64_t K, int64_t L,
                                                                 int32_t* __restrict__ g_idx,
                                                                 int32_t* __restrict__ invperm) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= K) return;
    const uint32_t p = (uint32_t)perm[i];
    if (p >= (uint32_t)K) return;                         // not a permutation: nothing is written through it
    if (g_idx) g_idx[p] = (int32_t)(i / L);
    if (invperm) invperm[p] = (int32_t)i;
}

// one workgroup: *status = 0, or 1 + the first i with idx[i] outside [0, bound)
__global__ __launch_bounds__(1024) void awq_gptq_check_index_kernel(const int32_t* __restrict__ idx, int64_t n,
                                                                    uint32_t bound, int32_t* __restrict__ status) {
    __shared__ unsigned long long first[1024];
    unsigned long long mine = ~0ull;
    for (int64_t i = threadIdx.x; i < n; i += 1024)
        if ((uint32_t)idx[i] >= bound && (unsigned long long)i < mine) mine = (unsigned long long)i;
    first[threadIdx.x] = mine;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && first[threadIdx.x + s] < first[threadIdx.x]) first[threadIdx.x] = first[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *status = first[0] == ~0ull ? 0 : (int32_t)(first[0] + 1);
}

// fp16 bits h -> the output element: OUT 0 = bf16 (RNE of the fp16 value; a NaN is 0x7FC0), 1 = fp16
// bits, 2 = fp32 (the widened value)
template <int OUT> struct OutElem;
template <> struct OutElem<AWQ_DTYPE_BF16> {
    typedef uint16_t type;
    static __device__ __forceinline__ uint16_t of(uint16_t h) {
        const float f = (float)__builtin_bit_cast(_Float16, h);
        if (f != f) return 0x7FC0u;
        const uint32_t u = __float_as_uint(f);
        return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
    }
};
template <> struct OutElem<AWQ_DTYPE_F16> {
    typedef uint16_t type;
    static __device__ __forceinline__ uint16_t of(uint16_t h) { return h; }
};
template <> struct OutElem<AWQ_DTYPE_F32> {
    typedef float type;
    static __device__ __forceinline__ float of(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
};

// PAIR: out is aligned to two elements, so a lane stores its dword's two results at once
template <int OUT, bool PAIR>
__global__ __launch_bounds__(256) void awq_gptq_dequant_kernel(const uint32_t* __restrict__ qweight_t,
                                                               const uint32_t* __restrict__ qzeros_t,
                                                               const uint16_t* __restrict__ scales_t,
                                                               const int32_t* __restrict__ g_idx, int64_t N, int64_t K,
                                                               uint32_t G, int off, int64_t tk,
                                                               typename OutElem<OUT>::type* __restrict__ out) {
    typedef typename OutElem<OUT>::type T;
    __shared__ uint32_t tile[kDN][kDStride];
    const int64_t b = blockIdx.x;
    const int64_t k0 = (b % tk) * kDK, n0 = (b / tk) * kDN;   // k tiles fastest: neighbours extend the same output rows
    const int64_t R = K / 8, wn = N / 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = n0 + lane;
    const bool live = n < N;
    const int64_t nc = live ? n : N - 1;                  // (a lane past N reads a valid address and stores nothing)
    const int zsh = 4 * (int)(nc & 7);

    uint32_t words[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t r = k0 / 8 + 4 * wave + j;
        words[j] = r < R ? qweight_t[r * N + nc] : 0u;
    }
    uint32_t gcur = 0xFFFFFFFFu;
    float scur = 0.f;
    int zcur = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t r = k0 / 8 + 4 * wave + j;
        if (r >= R) break;                                // wave-uniform
        uint32_t g[8];
        bool same = true;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t v = (uint32_t)__builtin_amdgcn_readfirstlane(g_idx[8 * r + i]);
            g[i] = v < G ? v : 0u;                        // out of range: group 0
            same = same && g[i] == gcur;
        }
        float s[8];
        int z[8];
        if (same) {
#pragma unroll
            for (int i = 0; i < 8; ++i) { s[i] = scur; z[i] = zcur; }
        } else {
            uint16_t sb[8];
            uint32_t zw[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                sb[i] = scales_t[(int64_t)g[i] * N + nc];
                zw[i] = qzeros_t[(int64_t)g[i] * wn + (nc >> 3)];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                s[i] = (float)__builtin_bit_cast(_Float16, sb[i]);
                z[i] = (int)(((zw[i] >> zsh) + (uint32_t)off) & 15u);
            }
            gcur = g[7]; scur = s[7]; zcur = z[7];
        }
        uint16_t h[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            // (u - z') is an integer of magnitude <= 15 and s an fp16: the fp32 product is exact, and
            // one RNE conversion gives fp16(fp16(u - z') s)
            const float p = (float)((int)((words[j] >> (4 * i)) & 15u) - z[i]) * s[i];
            h[i] = __builtin_bit_cast(uint16_t, (_Float16)p);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[lane][4 * (4 * wave + j) + i] = (uint32_t)h[2 * i] | ((uint32_t)h[2 * i + 1] << 16);
    }
    __syncthreads();
    const int64_t k = k0 + 2 * lane;
    if (k >= K) return;                                   // (K % 8 == 0: a pair is wholly inside or outside)
#pragma unroll 4
    for (int p = 0; p < kDN / 4; ++p) {
        const int row = wave + 4 * p;
        if (n0 + row >= N) break;
        const uint32_t v = tile[row][lane];
        T* dst = out + (n0 + row) * K + k;
        const T a = OutElem<OUT>::of((uint16_t)v), c = OutElem<OUT>::of((uint16_t)(v >> 16));
        if constexpr (PAIR) {
            typedef T T2 __attribute__((ext_vector_type(2)));
            __builtin_nontemporal_store((T2){a, c}, (T2*)dst);
        } else {
            dst[0] = a;
            dst[1] = c;
        }
    }
}

template <int OUT>
hipError_t launch_dequant_gptq(const int32_t* qweight_t, const int32_t* qzeros_t, const uint16_t* scales_t,
                               const int32_t* g_idx, int64_t N, int64_t K, int64_t G, int off, void* out,
                               hipStream_t stream) {
    typedef typename OutElem<OUT>::type T;
    const int64_t tk = (K + kDK - 1) / kDK, tn = (N + kDN - 1) / kDN;
    const bool pair = aligned(out, 2 * sizeof(T));
    const auto kernel = pair ? awq_gptq_dequant_kernel<OUT, true> : awq_gptq_dequant_kernel<OUT, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(tk * tn)), dim3(256), 0, stream, (const uint32_t*)qweight_t,
                       (const uint32_t*)qzeros_t, scales_t, g_idx, N, K, (uint32_t)G, off, tk, (T*)out);
    return hipPeekAtLastError();
}

}  // namespace
}  // namespace awq

extern "C" int awq_gptq_permute_rows(const int32_t* qweight_t_in, const int32_t* src, int64_t N, int64_t K,
                                     int32_t* qweight_t_out, void* stream) {
    using namespace awq;
    set_error(AWQ_OK, "");
    if (N < 0 || K < 0) return fail(AWQ_EINVAL, "negative size (N=%lld, K=%lld)", (long long)N, (long long)K);
    if (N % 8 != 0 || K % 8 != 0)
        return fail(AWQ_EINVAL, "GPTQ layout needs out_features %% 8 == 0 and in_features %% 8 == 0 (N=%lld, K=%lld)",
                    (long long)N, (long long)K);
    if (N == 0 || K == 0) return AWQ_OK;
    if (K >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31) || N * K > ((int64_t)1 << 42))
        return fail(AWQ_EUNSUPPORTED, "GPTQ act-order: N and K are limited to 2^31 - 1 and N * K to 2^42 (N=%lld, K=%lld)",
                    (long long)N, (long long)K);
    if (!qweight_t_in || !src || !qweight_t_out) return fail(AWQ_EINVAL, "null argument");
    if (!aligned(qweight_t_in, 4) || !aligned(src, 4) || !aligned(qweight_t_out, 4))
        return fail(AWQ_EINVAL, "misaligned argument (4-B alignment is needed)");
    if (qweight_t_in == qweight_t_out) return fail(AWQ_EINVAL, "the gather is not in place: qweight_t_out is qweight_t_in");
    const int64_t R = K / 8, strips = (N + kStripW - 1) / kStripW, chunks = (R + kStripR - 1) / kStripR;
    const int64_t grid = (strips + 7) / 8 * 8 * chunks;      // <= 2^42 / 8 / 64 / 64 + 8 chunks: below 2^31
    const bool vec = aligned(qweight_t_in, 16) && aligned(qweight_t_out, 16);
    hipLaunchKernelGGL(vec ? awq_gptq_permute_kernel<true> : awq_gptq_permute_kernel<false>, dim3((unsigned)grid),
                       dim3(256), 0, (hipStream_t)stream, (const uint32_t*)qweight_t_in, src, N, R, strips, chunks,
                       (uint32_t*)qweight_t_out);
    return hip_status(hipPeekAtLastError(), "awq gptq permute kernel");
}

extern "C" int awq_gptq_gidx_from_perm(const int32_t* perm, int64_t K, int64_t group_size, int32_t* g_idx,
                                       int32_t* invperm, void* stream) {
    using namespace awq;
    set_error(AWQ_OK, "");
    if (K < 0) return fail(AWQ_EINVAL, "negative size (K=%lld)", (long long)K);
    if (group_size <= 0) return fail(AWQ_EINVAL, "Group size must be a positive integer: %lld", (long long)group_size);
    if (K == 0) return AWQ_OK;
    if (K >= ((int64_t)1 << 31)) return fail(AWQ_EUNSUPPORTED, "GPTQ act-order: K is limited to 2^31 - 1 (K=%lld)", (long long)K);
    if (!perm) return fail(AWQ_EINVAL, "null argument: perm");
    if (!g_idx && !invperm) return fail(AWQ_EINVAL, "null argument: at least one output is needed");
    if (!aligned(perm, 4) || !aligned(g_idx, 4) || !aligned(invperm, 4))
        return fail(AWQ_EINVAL, "misaligned argument (4-B alignment is needed)");
    hipLaunchKernelGGL(awq_gptq_gidx_perm_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       perm, K, group_size, g_idx, invperm);
    return hip_status(hipPeekAtLastError(), "awq gptq g_idx kernel");
}

extern "C" int awq_gptq_check_index(const int32_t* idx, int64_t n, int64_t bound, int32_t* status, void* stream) {
    using namespace awq;
    set_error(AWQ_OK, "");
    if (n < 0 || bound < 0) return fail(AWQ_EINVAL, "negative size (n=%lld, bound=%lld)", (long long)n, (long long)bound);
    if (n >= ((int64_t)1 << 31) || bound >= ((int64_t)1 << 31))
        return fail(AWQ_EUNSUPPORTED, "index check: n and bound are limited to 2^31 - 1 (n=%lld, bound=%lld)",
                    (long long)n, (long long)bound);
    if (!status || (n > 0 && !idx)) return fail(AWQ_EINVAL, "null argument");
    if (!aligned(idx, 4) || !aligned(status, 4)) return fail(AWQ_EINVAL, "misaligned argument (4-B alignment is needed)");
    hipLaunchKernelGGL(awq_gptq_check_index_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, idx, n, (uint32_t)bound,
                       status);
    return hip_status(hipPeekAtLastError(), "awq gptq index check kernel");
}

extern "C" int awq_dequantize_gptq(const int32_t* qweight_t, const int32_t* qzeros_t, const uint16_t* scales_t,
                                   const int32_t* g_idx, int64_t N, int64_t K, int64_t G, int zero_offset, void* out,
                                   int out_dtype, void* stream) {
    using namespace awq;
    set_error(AWQ_OK, "");
    if (N < 0 || K < 0 || G < 0)
        return fail(AWQ_EINVAL, "negative size (N=%lld, K=%lld, G=%lld)", (long long)N, (long long)K, (long long)G);
    if (N % 8 != 0 || K % 8 != 0)
        return fail(AWQ_EINVAL, "GPTQ layout needs out_features %% 8 == 0 and in_features %% 8 == 0 (N=%lld, K=%lld)",
                    (long long)N, (long long)K);
    if (zero_offset != 0 && zero_offset != 1)
        return fail(AWQ_EINVAL, "zero_offset must be 0 (gptq_v2) or 1 (gptq): %d", zero_offset);
    if (out_dtype != AWQ_DTYPE_F32 && out_dtype != AWQ_DTYPE_F16 && out_dtype != AWQ_DTYPE_BF16)
        return fail(AWQ_EUNSUPPORTED, "awq_dequantize_gptq writes fp32, fp16 or bf16 (out_dtype=%d)", out_dtype);
    if (N == 0 || K == 0) return AWQ_OK;
    if (G == 0) return fail(AWQ_EINVAL, "a non-empty weight needs at least one group (G=0)");
    if (K >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31) || G >= ((int64_t)1 << 31) || N * K > ((int64_t)1 << 42))
        return fail(AWQ_EUNSUPPORTED, "GPTQ act-order: N, K and G are limited to 2^31 - 1 and N * K to 2^42 (N=%lld, "
                                      "K=%lld, G=%lld)", (long long)N, (long long)K, (long long)G);
    if (!qweight_t || !qzeros_t || !scales_t || !g_idx || !out) return fail(AWQ_EINVAL, "null argument");
    if (!aligned(qweight_t, 4) || !aligned(qzeros_t, 4) || !aligned(scales_t, 2) || !aligned(g_idx, 4) ||
        !aligned(out, out_dtype == AWQ_DTYPE_F32 ? 4 : 2))
        return fail(AWQ_EINVAL, "misaligned argument (words and fp32 need 4-B, 16-bit values 2-B alignment)");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (out_dtype == AWQ_DTYPE_F32) e = launch_dequant_gptq<AWQ_DTYPE_F32>(qweight_t, qzeros_t, scales_t, g_idx, N, K, G, zero_offset, out, s);
    else if (out_dtype == AWQ_DTYPE_F16) e = launch_dequant_gptq<AWQ_DTYPE_F16>(qweight_t, qzeros_t, scales_t, g_idx, N, K, G, zero_offset, out, s);
    else e = launch_dequant_gptq<AWQ_DTYPE_BF16>(qweight_t, qzeros_t, scales_t, g_idx, N, K, G, zero_offset, out, s);
    return hip_status(e, "awq gptq dequantize kernel");
}
