// awq_qerror.hip — quantization-error report (awq_quant_error, include/awq_hip.h): per-group
// sum |d|, sum d^2, sum w^2, max |d| and non-finite count of d = w - dequantize(packed result),
// read in ONE pass from the original weights and the packed qweight / qzeros / scales, then the
// per-tensor fp64 totals.  Self-contained: the two entry points, their validation and kernels.
//
// Per element (the definition every implementation restates):
//   dq = fp32(fp16(fp16(q - z) * s))   (awq.py:459-539; q - z = field(qweight) - field(qzeros):
//        an integer of at most 9 bits, exact in fp16; times an fp16 scale the product has at most
//        19 significand bits, exact in f32, so ONE RNE conversion to fp16 is RN_f16 of the product)
//   d = RN_f32(w - dq), a = |d|, e = RN_f32(d d), p = RN_f32(w w); the element is non-finite when
//   d, e or p is NaN / inf (e = d d is then NaN / inf too: the test is on e and p) and then adds
//   nothing but 1 to the group's count.
// Per group (fp32): each 8-element chunk summed in element order from +0, then the pairwise tree
// over 64 chunk slots, adjacent pairs first — the clip search's canonical order (awq_quantize_search),
// which the xor butterfly over a group's lanes reproduces (fp addition commutes; every partial
// is >= +0, so the empty slots' zeros change nothing).
#include <algorithm>

#include "awq_quant.h"

namespace awq {
namespace {

constexpr int kMaxGroup = 512;             // 64 chunk slots of 8 elements
constexpr int kGroupBlock2 = 1024;         // groups per level-2 block (= awq_act_search_select's)
constexpr int64_t kMaxBlocks2 = 6144 * 32; // blocks awq_act_search_select's last level takes

// The statistics of one chunk's elements, accumulated in element order.
struct Acc {
    float a = 0.0f, e = 0.0f, p = 0.0f, m = 0.0f;
    int bad = 0;
    // w: the weight as fp32; diff = q - z; s: the fp16 scale's value
    __device__ __forceinline__ void add(float w, int diff, float s) {
        const float dq = (float)(_Float16)((float)diff * s);   // exact product, one RNE to fp16
        const float d = w - dq;
        const float ab = __builtin_fabsf(d), sq = d * d, ww = w * w;
        const bool fin = sq < __builtin_inff() && ww < __builtin_inff();   // NaN compares false
        a = a + (fin ? ab : 0.0f);
        e = e + (fin ? sq : 0.0f);
        p = p + (fin ? ww : 0.0f);
        m = __builtin_fmaxf(m, fin ? ab : 0.0f);
        bad += fin ? 0 : 1;
    }
};

// Fields 2t, 2t+1 of a chunk's qweight word(s) as the fp16 pair (1024 + f0, 1024 + f1): at 2^10
// fp16's ulp is 1, so 1024 + f (f < 1024) is the bit pattern 0x6400 + f.
template <int BITS, int QW>
__device__ __forceinline__ h2v field_pair(const uint32_t (&qw)[QW], int t) {
    uint32_t lo, hi;
    if (BITS == 4) {
        const uint32_t x = qw[0] >> (8 * t);
        lo = x & 0xFu;
        hi = (x << 12) & 0xF0000u;
    } else {
        const uint32_t x = qw[t >> 1] >> (16 * (t & 1));
        lo = x & 0xFFu;
        hi = (x << 8) & 0xFF0000u;
    }
    return __builtin_bit_cast(h2v, lo | hi | 0x64006400u);
}

// One chunk with no test per element (the streaming kernel's common case): q - z and the product
// with the scale as packed fp16 ops, two elements each — (1024 + f) - (1024 + z) is exact, the
// packed multiply is the definition's fp16(fp16(q - z) * s) itself — and unmasked sums.  A
// non-finite element leaves the chunk's sum of e or p NaN / inf (the terms are >= 0), which the
// caller tests once per chunk; such a wave redoes its tile with Acc::add.
template <typename F, int BITS, int QW>
__device__ __forceinline__ void chunk_fast(const Chunk<F::NW>& v, const uint32_t (&qw)[QW], h2v zq, h2v s2, Acc& c) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const h2v dq = (field_pair<BITS, QW>(qw, t) - zq) * s2;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float w = F::elem(v, 2 * t + u);
            const float d = w - (float)(u ? dq.y : dq.x);
            c.a = c.a + __builtin_fabsf(d);
            c.e = c.e + d * d;
            c.p = c.p + w * w;
            c.m = __builtin_fmaxf(c.m, __builtin_fabsf(d));
        }
    }
}

// ---------------------------------------------------------------------------------------
// Streaming kernel: group_size GS in {32, 64, 128, 256}, K % GS == 0, 16-B aligned w / qweight,
// so the tensor is a flat run of groups and qweight a flat run of words.  One wave per
// 2048-element tile (awq_internal.h): load j of 4 covers the tile's elements [512 j, 512 (j+1)),
// lane l its 8 elements at 8 l — chunk l % L of group slot j * (64 / L) + l / L (L = GS / 8) —
// as one 16-B nt load (two for fp32) plus the chunk's qweight word (two at 8 bits).  Lane l also
// owns the parameters of ONE group, slot (l & 3) * (64 / L) + l / L: one scales and one qzeros
// load instruction per tile, handed to the group's lanes for load j by a quad broadcast of
// lane j's value; the same lanes (l % L < 4) store that group's results.  Slots past the tensor's
// end fall outside the buffer descriptors' range (zeros) and are not stored.  The arithmetic runs
// without a test per element first (chunk_fast) and again with it (Acc::add) in the waves that
// hold a non-finite element: the same bits where nothing is non-finite.
// ---------------------------------------------------------------------------------------
template <typename F, int BITS, int GS>
__global__ __launch_bounds__(64) void qerror_stream_kernel(const void* __restrict__ w,
                                                           const uint32_t* __restrict__ qweight,
                                                           const uint32_t* __restrict__ qzeros,
                                                           const uint16_t* __restrict__ scales, int64_t n_elems,
                                                           int64_t n_groups, uint32_t G, uint32_t zpr,
                                                           float* __restrict__ stats,
                                                           int32_t* __restrict__ nonfinite) {
    constexpr int L = GS / 8, S = kTileElems / GS, Q = S / 4, PER = 32 / BITS, QW = BITS / 4;
    constexpr uint32_t MASK = (1u << BITS) - 1u;
    const int lane = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t e0 = tile * kTileElems;
    const uint32_t te = (uint32_t)min((int64_t)kTileElems, n_elems - e0);   // elements of this tile
    const __amdgpu_buffer_rsrc_t rw = rsrc((const char*)w + e0 * F::kBytes, te * (uint32_t)F::kBytes);
    const __amdgpu_buffer_rsrc_t rq = rsrc((const char*)qweight + e0 * BITS / 8, te * (uint32_t)BITS / 8u);

    Chunk<F::NW> v[4];
    uint32_t qw[4][QW];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int h = 0; h < F::NW; ++h)
            v[j].w[h] = __builtin_amdgcn_raw_buffer_load_b128(
                rw, (uint32_t)(j * 512 * F::kBytes + lane * 8 * F::kBytes + 16 * h), 0, AWQ_LOAD_AUX);
        if constexpr (BITS == 4) {
            qw[j][0] = __builtin_amdgcn_raw_buffer_load_b32(rq, (uint32_t)(j * 256 + lane * 4), 0, AWQ_LOAD_AUX);
        } else {
            const u2v t = __builtin_amdgcn_raw_buffer_load_b64(rq, (uint32_t)(j * 512 + lane * 8), 0, AWQ_LOAD_AUX);
            qw[j][0] = t.x;
            qw[j][1] = t.y;
        }
    }

    // this lane's parameter group
    const uint32_t tg = te / GS;                                   // groups of this tile
    const uint32_t pslot = (uint32_t)(lane & 3) * Q + (uint32_t)lane / L;
    const bool powner = pslot < tg;
    const int64_t pg = tile * S + pslot;                           // flat group r * G + g
    uint32_t sbits = 0, zf = 0;
    if (powner) {
        sbits = scales[pg];
        const uint32_t r = (uint32_t)pg / G, g = (uint32_t)pg - r * G;   // n_groups < 2^31 (host-checked)
        const uint32_t zw = qzeros[(int64_t)r * zpr + g / PER];
        zf = (zw >> (BITS * (g % PER))) & MASK;
    }

    // fast pass: packed-fp16 dq, no per-element test; one test per chunk afterwards
    const uint32_t spack = sbits | (sbits << 16), zpack = (0x6400u + zf) * 0x10001u;
    Acc c[4];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        chunk_fast<F, BITS, QW>(v[j], qw[j], __builtin_bit_cast(h2v, bcast_u(j, zpack)),
                                __builtin_bit_cast(h2v, bcast_u(j, spack)), c[j]);
        ok = ok && c[j].e < __builtin_inff() && c[j].p < __builtin_inff();   // NaN compares false
    }
    float oa = 0.0f, oe = 0.0f, op = 0.0f;
    uint32_t om = 0;
    int ob = 0;
    if (__builtin_amdgcn_ballot_w64(!ok) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // the group's tree; a non-negative float's order is its bit pattern's
            const float ga = grp_sum<L>(c[j].a), ge = grp_sum<L>(c[j].e), gp = grp_sum<L>(c[j].p);
            const uint32_t gm = grp_max<L, uint32_t>(__float_as_uint(c[j].m));
            if ((lane & 3) == j) { oa = ga; oe = ge; op = gp; om = gm; }
        }
    } else {
        // a wave holding a non-finite element (or a chunk sum that overflowed): the exact pass
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = (float)__builtin_bit_cast(_Float16, (uint16_t)bcast_u(j, sbits));
            const int z = (int)bcast_u(j, zf);
            Acc x;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t word = BITS == 4 ? qw[j][0] : qw[j][(i >> 2) * (QW - 1)];
                const int f = (int)((word >> (BITS * (i % PER))) & MASK);
                x.add(F::elem(v[j], i), f - z, s);
            }
            const float ga = grp_sum<L>(x.a), ge = grp_sum<L>(x.e), gp = grp_sum<L>(x.p);
            const uint32_t gm = grp_max<L, uint32_t>(__float_as_uint(x.m));
            const int gb = grp_sum<L>(x.bad);
            if ((lane & 3) == j) { oa = ga; oe = ge; op = gp; om = gm; ob = gb; }
        }
    }
    if (powner && (lane % L) < 4) {
        stats[pg] = oa;
        stats[n_groups + pg] = oe;
        stats[2 * n_groups + pg] = op;
        stats[3 * n_groups + pg] = __uint_as_float(om);
        nonfinite[pg] = ob;
    }
}

// ---------------------------------------------------------------------------------------
// Generic kernel: any K, any group_size <= 512 (tail groups, partial chunks), element-aligned
// pointers.  One wave per group; lane l takes chunk l (the group's elements 8 l .. 8 l + 7 that
// exist) and the 64 lanes are the canonical tree's 64 chunk slots.
// ---------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ float load_elem(const void* w, int64_t i) {
    if (DT == AWQ_DTYPE_BF16) return __uint_as_float((uint32_t)((const uint16_t*)w)[i] << 16);
    if (DT == AWQ_DTYPE_F16) return (float)((const _Float16*)w)[i];
    return ((const float*)w)[i];
}

template <int DT>
__global__ __launch_bounds__(256) void qerror_group_kernel(const void* __restrict__ w,
                                                           const uint32_t* __restrict__ qweight,
                                                           const uint32_t* __restrict__ qzeros,
                                                           const uint16_t* __restrict__ scales, int64_t K, int64_t gs,
                                                           int64_t G, int bits, int64_t n_groups,
                                                           float* __restrict__ stats, int32_t* __restrict__ nonfinite) {
    const int per = 32 / bits;
    const uint32_t mask = (1u << bits) - 1u;
    const int64_t wpr = (K + per - 1) / per, zpr = (G + per - 1) / per;
    const int lane = threadIdx.x & 63;
    for (int64_t gi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); gi < n_groups; gi += (int64_t)gridDim.x * 4) {
        const int64_t r = gi / G, g = gi - r * G, k0 = g * gs;
        const int n = (int)min(gs, K - k0);
        const float s = (float)__builtin_bit_cast(_Float16, scales[gi]);
        const int z = (int)((qzeros[r * zpr + g / per] >> (bits * (int)(g % per))) & mask);
        Acc c;
        for (int i = 0; i < 8; ++i) {
            const int kk = lane * 8 + i;
            if (kk < n) {
                const int64_t k = k0 + kk;
                const int f = (int)((qweight[r * wpr + k / per] >> (bits * (int)(k % per))) & mask);
                c.add(load_elem<DT>(w, r * K + k), f - z, s);
            }
        }
        const float ga = wave_sum(c.a), ge = wave_sum(c.e), gp = wave_sum(c.p);
        const int gb = wave_sum(c.bad);
        float gm = c.m;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) gm = __builtin_fmaxf(gm, __shfl_xor(gm, o, 64));
        if (lane == 0) {
            stats[gi] = ga;
            stats[n_groups + gi] = ge;
            stats[2 * n_groups + gi] = gp;
            stats[3 * n_groups + gi] = gm;
            nonfinite[gi] = gb;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Level 2.  The three fp64 sums are awq_act_search_select's (launch_act_select with the
// three planes of group_stats as its candidates); the max and the count are order-free: one
// workgroup per 1024 groups, then one workgroup over the blocks.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void block_max_sum(float& m, double& c) {
    __shared__ float sm[4];
    __shared__ double sc[4];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        m = __builtin_fmaxf(m, __shfl_xor(m, o, 64));
        c = c + __shfl_xor(c, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sm[threadIdx.x >> 6] = m;
        sc[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    m = __builtin_fmaxf(__builtin_fmaxf(sm[0], sm[1]), __builtin_fmaxf(sm[2], sm[3]));
    c = (sc[0] + sc[1]) + (sc[2] + sc[3]);   // integers below 2^53: exact in any order
}

__global__ __launch_bounds__(256) void qerror_block_kernel(const float* __restrict__ gmax,
                                                           const int32_t* __restrict__ nonfinite, int64_t n_groups,
                                                           double* __restrict__ wmax, double* __restrict__ wcnt) {
    const int64_t g0 = (int64_t)blockIdx.x * kGroupBlock2;
    float m = 0.0f;
    double c = 0.0;
    for (int i = threadIdx.x; i < kGroupBlock2; i += 256)
        if (g0 + i < n_groups) {
            m = __builtin_fmaxf(m, gmax[g0 + i]);
            c += (double)nonfinite[g0 + i];
        }
    block_max_sum(m, c);
    if (threadIdx.x == 0) {
        wmax[blockIdx.x] = (double)m;
        wcnt[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(256) void qerror_final_kernel(const double* __restrict__ wmax,
                                                           const double* __restrict__ wcnt, int64_t nblk,
                                                           double* __restrict__ totals) {
    float m = 0.0f;
    double c = 0.0;
    for (int64_t i = threadIdx.x; i < nblk; i += 256) {
        m = __builtin_fmaxf(m, (float)wmax[i]);
        c += wcnt[i];
    }
    block_max_sum(m, c);
    if (threadIdx.x == 0) {
        totals[3] = (double)m;
        totals[4] = c;
    }
}

int64_t level2_blocks(int64_t n_groups) { return (n_groups + kGroupBlock2 - 1) / kGroupBlock2; }

// shape limits shared by both entry points: 0 = fine
int check_shape(int64_t rows, int64_t K, int64_t group_size) {
    if (group_size <= 0) return fail(AWQ_EINVAL, "Group size must be a positive integer: %lld", (long long)group_size);
    if (rows < 0 || K < 0) return fail(AWQ_EINVAL, "negative shape (%lld, %lld)", (long long)rows, (long long)K);
    if (group_size > kMaxGroup)
        return fail(AWQ_EUNSUPPORTED, "awq_quant_error: group_size %lld > 512 (64 chunks of 8) is not supported",
                    (long long)group_size);
    const int64_t G = (K + group_size - 1) / group_size;
    if (rows > 0 && G > 0 && (G > (int64_t)0x7FFFFFFF / rows || level2_blocks(rows * G) > kMaxBlocks2 ||
                              K > ((int64_t)1 << 40) / rows))
        return fail(AWQ_EUNSUPPORTED, "awq_quant_error: %lld x %lld groups exceed the level-2 reduce's range",
                    (long long)rows, (long long)G);
    return AWQ_OK;
}

template <typename F, int BITS>
void launch_stream(int gs, unsigned tiles, hipStream_t st, const void* w, const uint32_t* qweight,
                   const uint32_t* qzeros, const uint16_t* scales, int64_t n, int64_t ng, uint32_t G, uint32_t zpr,
                   float* stats, int32_t* nonfinite) {
#define AWQ_QE(GS)                                                                                                  \
    hipLaunchKernelGGL((qerror_stream_kernel<F, BITS, GS>), dim3(tiles), dim3(64), 0, st, w, qweight, qzeros, scales, \
                       n, ng, G, zpr, stats, nonfinite)
    switch (gs) {
    case 32: AWQ_QE(32); break;
    case 64: AWQ_QE(64); break;
    case 128: AWQ_QE(128); break;
    default: AWQ_QE(256); break;
    }
#undef AWQ_QE
}

}  // namespace
}  // namespace awq

using namespace awq;

extern "C" int64_t awq_quant_error_work_bytes(int64_t rows, int64_t K, int64_t group_size) {
    if (check_shape(rows, K, group_size) != AWQ_OK) return -1;
    const int64_t G = (K + group_size - 1) / group_size;
    const int64_t nblk = level2_blocks(rows * G);
    return 8 * 5 * (nblk > 0 ? nblk : 1);   // 3 sum planes (awq_act_search_select's work), max, count
}

extern "C" int awq_quant_error(const void* w, int dtype, int64_t rows, int64_t K, int64_t group_size, int bits,
                               int symmetric, const int32_t* qweight, const int32_t* qzeros, const uint16_t* scales,
                               float* group_stats, int32_t* group_nonfinite, double* work, double* totals,
                               void* stream) {
    (void)symmetric;   // q - z = field(qweight) - field(qzeros): qmin cancels
    if (bits != 4 && bits != 8) return fail(AWQ_EINVAL, "Unsupported bit width: %d. Supported: 4, 8.", bits);
    if (int rc = check_shape(rows, K, group_size)) return rc;
    if (dtype == AWQ_DTYPE_F64) return fail(AWQ_EUNSUPPORTED, "awq_quant_error: fp64 weights are not supported");
    if (dtype != AWQ_DTYPE_BF16 && dtype != AWQ_DTYPE_F16 && dtype != AWQ_DTYPE_F32)
        return fail(AWQ_EINVAL, "awq_quant_error: dtype code %d is not a weight dtype (bf16, fp16, fp32)", dtype);
    const int64_t n = rows * K;
    const int64_t G = (K + group_size - 1) / group_size, ng = rows * G;
    if (n > 0 && (!w || !qweight || !qzeros || !scales || !group_stats || !group_nonfinite))
        return fail(AWQ_EINVAL, "awq_quant_error: null argument");
    if (totals && !work) return fail(AWQ_EINVAL, "awq_quant_error: totals needs the workspace");
    const size_t esz = dtype == AWQ_DTYPE_F32 ? 4 : 2;
    if (!aligned(w, esz) || !aligned(qweight, 4) || !aligned(qzeros, 4) || !aligned(scales, 2) ||
        !aligned(group_stats, 4) || !aligned(group_nonfinite, 4) || !aligned(work, 8) || !aligned(totals, 8))
        return fail(AWQ_EINVAL, "awq_quant_error: a pointer is not aligned to its element size");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (n == 0) {
        if (totals) e = hipMemsetAsync(totals, 0, 5 * sizeof(double), st);
        return e == hipSuccess ? AWQ_OK : set_error(AWQ_EHIP, hipGetErrorString(e));
    }
    const uint32_t* qwp = (const uint32_t*)qweight;
    const uint32_t* qzp = (const uint32_t*)qzeros;
    const int64_t tiles = (n + kTileElems - 1) / kTileElems;
    if (fast_group_size(group_size) && K % group_size == 0 && aligned(w, 16) && aligned(qweight, 16) &&
        tiles < (int64_t)0x7FFFFFFF) {
        const uint32_t zpr = (uint32_t)((G * bits + 31) / 32);
#define AWQ_QE_FMT(F)                                                                                              \
    if (bits == 4) launch_stream<F, 4>((int)group_size, (unsigned)tiles, st, w, qwp, qzp, scales, n, ng, (uint32_t)G, \
                                       zpr, group_stats, group_nonfinite);                                         \
    else launch_stream<F, 8>((int)group_size, (unsigned)tiles, st, w, qwp, qzp, scales, n, ng, (uint32_t)G, zpr,    \
                             group_stats, group_nonfinite);
        if (dtype == AWQ_DTYPE_BF16) { AWQ_QE_FMT(FmtBF16) }
        else if (dtype == AWQ_DTYPE_F16) { AWQ_QE_FMT(FmtF16) }
        else { AWQ_QE_FMT(FmtF32) }
#undef AWQ_QE_FMT
    } else {
        const unsigned grid = diag_cap((unsigned)std::min<int64_t>((ng + 3) / 4, (int64_t)256 * 64));
#define AWQ_QE_GEN(DT)                                                                                         \
    hipLaunchKernelGGL((qerror_group_kernel<DT>), dim3(grid), dim3(256), 0, st, w, qwp, qzp, scales, K, group_size, \
                       G, bits, ng, group_stats, group_nonfinite)
        if (dtype == AWQ_DTYPE_BF16) AWQ_QE_GEN(AWQ_DTYPE_BF16);
        else if (dtype == AWQ_DTYPE_F16) AWQ_QE_GEN(AWQ_DTYPE_F16);
        else AWQ_QE_GEN(AWQ_DTYPE_F32);
#undef AWQ_QE_GEN
    }
    e = hipPeekAtLastError();
    if (e == hipSuccess && totals) {
        const int64_t nblk = level2_blocks(ng);
        e = launch_act_select(group_stats, 3, ng, nullptr, 0, work, totals, nullptr, nullptr, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(qerror_block_kernel, dim3((unsigned)nblk), dim3(256), 0, st, group_stats + 3 * ng,
                               group_nonfinite, ng, work + 3 * nblk, work + 4 * nblk);
            hipLaunchKernelGGL(qerror_final_kernel, dim3(1), dim3(256), 0, st, work + 3 * nblk, work + 4 * nblk, nblk,
                               totals);
            e = hipPeekAtLastError();
        }
    }
    return hip_status(e, "awq quant error kernels");
}
