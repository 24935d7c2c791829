// awq_gptq_round.hip — GPTQ error-compensated rounding of one block of input columns
// (include/awq_hip.h awq_gptq_round_block).
//
// The in-block loop of GPTQ is a chain: column i of a row is rounded, its error e, divided by the
// inverse factor's diagonal, is taken off every later column of the block through row i of the
// factor, and only then can column i + 1 be rounded.  Rows do not meet.  So one lane owns one row:
// the block's up to 128 working values stay in 128 VGPRs for the whole chain, row i of the factor
// is an LDS broadcast read (every lane reads the same address), and the update of the later columns
// is v_pk_mul_f32 / v_pk_add_f32 on register pairs.  The chain is unrolled completely (every
// register index is a constant); bits, symmetric and group_size are wave-uniform run-time values,
// so there is one kernel, not one per combination.
//
// One 64-lane workgroup per 64 rows; it stages the upper triangle of the block's 128 x 128 piece of
// the factor in 64 KiB of LDS first.  The grid is one workgroup per 64 rows and not capped (N < 2^31
// rows: below 2^25 workgroups).
//
// Arithmetic: every operation below is a single fp32 operation rounded on its own (the Makefile
// builds with -ffp-contract=off; divisions are IEEE, -fhip-fp32-correctly-rounded-divide-sqrt), so a
// NumPy float32 restatement (tests/gptq_round_ref.py) gives the same bits.
#include "awq_quant.h"

namespace awq {
namespace {

constexpr int kBlock = 128;   // widest column block: a lane's register window
constexpr int kStep = 32;     // smallest group size: what the chain is cut into
constexpr int kBatch = 8;     // register pairs per batch of the update (16 factor values in flight, twice)

struct RoundMode {            // wave-uniform
    int gs, bits, sym;
    float qmin, qmax;         // the field range as q: [0, 2^bits - 1] or [-2^(bits-1), 2^(bits-1) - 1]
    int qmin_i;
    uint32_t nan_field;       // (INT32_MIN - qmin) & mask: the field of a NaN element (include/awq_hip.h)
    uint32_t nan_code;
};

struct RoundState {           // per lane, carried from a group's first column to its last
    float s;                  // (float)fp16(scale): what a reader dequantizes with
    float z;                  // zero point (0 when symmetric; NaN in a NaN group)
    uint32_t acc;             // fields of the qweight word being filled
    float e[4];               // errors of the 16-B err store being filled
};

__device__ __forceinline__ float elem(const f2 (&w)[kBlock / 2], int i) { return (i & 1) ? w[i >> 1].y : w[i >> 1].x; }

__device__ __forceinline__ GroupParams round_params(const RoundMode& m, float mn, float mx) {
    if (m.bits == 4) return m.sym ? params_from_range<FmtF32, 4, true>(mn, mx) : params_from_range<FmtF32, 4, false>(mn, mx);
    return m.sym ? params_from_range<FmtF32, 8, true>(mn, mx) : params_from_range<FmtF32, 8, false>(mn, mx);
}
__device__ __forceinline__ uint32_t round_zero_field(const RoundMode& m, float z) {
    if (m.bits == 4) return m.sym ? zero_field<4, true>(z) : zero_field<4, false>(z);
    return m.sym ? zero_field<8, true>(z) : zero_field<8, false>(z);
}

template <int P0>
__device__ __forceinline__ void load_batch(const float* ur, f2 (&ub)[kBatch]) {
#pragma unroll
    for (int k = 0; k < kBatch; ++k)
        if (P0 + k < kBlock / 2) ub[k] = *(const f2*)(ur + 2 * (P0 + k));
}

// column I of the block (a template constant: every register index below is one)
template <int I>
__device__ __forceinline__ void round_step(f2 (&w)[kBlock / 2], RoundState& st, const RoundMode& m, const float* su,
                                           bool live, int64_t row, int64_t K, int64_t c0, int n_cols, float* err,
                                           uint32_t* qweight, uint32_t* qzeros, uint16_t* scales) {
    constexpr int i = I, C = I / kStep;
    {
        if (I % kStep == 0 && (i % m.gs) == 0) {
            // the group's parameters from its working values as they stand now: the project's fp32
            // rule (raw-bits extremes -> group_range -> params_from_range)
            int smax = INT32_MIN;
            uint32_t umax = 0u, cmax = 0u;
#pragma unroll
            for (int c = C; c < kBlock / kStep; ++c) {
                if (c * kStep < i + m.gs) {
#pragma unroll
                    for (int k = c * kStep; k < (c + 1) * kStep; ++k) {
                        const uint32_t b = __float_as_uint(elem(w, k));
                        smax = max(smax, (int)b);
                        umax = max(umax, b);
                        cmax = max(cmax, ~b);
                    }
                }
            }
            float mn, mx;
            bool gnan;
            if (m.sym) group_range<FmtF32, true>(smax, umax, ~cmax, mn, mx, gnan);
            else group_range<FmtF32, false>(smax, umax, ~cmax, mn, mx, gnan);
            const GroupParams p = round_params(m, mn, mx);
            st.s = FmtF32::dq_scale(p.s);
            st.z = p.z;
            if (live) {
                const int64_t G = K / m.gs, g = (c0 + i) / m.gs;
                scales[row * G + g] = f16_bits(p.s, gnan, m.nan_code);
                // the group's zero field alone: the other fields of the word belong to other blocks
                const int per = 32 / m.bits;
                const int64_t wz = (G + per - 1) / per;
                uint32_t* zw = qzeros + row * wz + g / per;
                const int sh = m.bits * (int)(g % per);
                const uint32_t mask = ((1u << m.bits) - 1u) << sh;
                *zw = (*zw & ~mask) | (round_zero_field(m, p.z) << sh);
            }
        }
        // quantize and dequantize column i against s
        const float wi = elem(w, i);
        const float quo = wi / st.s;
        const float r = __builtin_rintf(quo) + st.z;
        const bool rnan = __builtin_isnan(r);
        const float qf = __builtin_fminf(__builtin_fmaxf(r, m.qmin), m.qmax);   // (NaN: qmin, unused)
        const uint32_t field = rnan ? m.nan_field : (uint32_t)((int)qf - m.qmin_i);
        const float dq = rnan ? r : (qf - st.z) * st.s;
        float e = (wi - dq) / su[i * kBlock + i];
        if (!(__builtin_isfinite(st.s) && __builtin_isfinite(dq) && __builtin_isfinite(quo))) e = 0.0f;
        // the field into its qweight word
        if (m.bits == 4) {
            st.acc = (i & 7) ? st.acc | (field << (4 * (i & 7))) : field;
            if ((i & 7) == 7 && live) qweight[row * (K >> 3) + ((c0 + i) >> 3)] = st.acc;
        } else {
            st.acc = (i & 3) ? st.acc | (field << (8 * (i & 3))) : field;
            if ((i & 3) == 3 && live) qweight[row * (K >> 2) + ((c0 + i) >> 2)] = st.acc;
        }
        st.e[i & 3] = e;
        if ((i & 3) == 3 && live)
            *(float4*)(err + row * n_cols + (i - 3)) = make_float4(st.e[0], st.e[1], st.e[2], st.e[3]);
        // take e U[c][c + 1 ..] off the later columns: product and difference rounded separately.
        // Batches of 8 register pairs, the next batch's LDS reads issued before this batch's
        // arithmetic; the scheduling barriers keep the compiler from hoisting every read of the
        // step (and of later steps) to its top, which spills the working values.
        const float* ur = su + i * kBlock;
        if ((i & 1) == 0) w[i >> 1].y = w[i >> 1].y - e * ur[i + 1];
        const f2 ev = {e, e};
        constexpr int P0 = (I >> 1) + 1, NB = (kBlock / 2 - P0 + kBatch - 1) / kBatch;
        f2 ub[2][kBatch];
        if constexpr (NB > 0) load_batch<P0>(ur, ub[0]);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b + 1 < NB) {
#pragma unroll
                for (int k = 0; k < kBatch; ++k)
                    if (P0 + (b + 1) * kBatch + k < kBlock / 2)
                        ub[(b + 1) & 1][k] = *(const f2*)(ur + 2 * (P0 + (b + 1) * kBatch + k));
            }
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const int jp = P0 + b * kBatch + k;
                if (jp < kBlock / 2) w[jp] = pk_add(w[jp], -pk_mul(ev, ub[b & 1][k]));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // every later column is up to date before the next step begins: an update of a far column is
        // not needed for a long time, and left alone the compiler defers it past the uniform
        // branches, keeping e and the factor's values alive (in scratch) until then
#pragma unroll
        for (int jp = I >> 1; jp < kBlock / 2; ++jp) asm volatile("" : "+v"(w[jp]));
        __builtin_amdgcn_sched_barrier(0);
    }
}

// columns [I, END) of the block
template <int I, int END>
__device__ __forceinline__ void round_steps(f2 (&w)[kBlock / 2], RoundState& st, const RoundMode& m, const float* su,
                                            bool live, int64_t row, int64_t K, int64_t c0, int n_cols, float* err,
                                            uint32_t* qweight, uint32_t* qzeros, uint16_t* scales) {
    if constexpr (I < END) {
        round_step<I>(w, st, m, su, live, row, K, c0, n_cols, err, qweight, qzeros, scales);
        round_steps<I + 1, END>(w, st, m, su, live, row, K, c0, n_cols, err, qweight, qzeros, scales);
    }
}
template <int C>
__device__ __forceinline__ void round_chunk(f2 (&w)[kBlock / 2], RoundState& st, const RoundMode& m, const float* su,
                                            bool live, int64_t row, int64_t K, int64_t c0, int n_cols, float* err,
                                            uint32_t* qweight, uint32_t* qzeros, uint16_t* scales) {
    round_steps<C * kStep, (C + 1) * kStep>(w, st, m, su, live, row, K, c0, n_cols, err, qweight, qzeros, scales);
}

__global__ __launch_bounds__(64) void awq_gptq_round_kernel(float* __restrict__ work, int64_t N, int64_t K, RoundMode m,
                                                           const float* __restrict__ u, int64_t c0, int n_cols,
                                                           float* __restrict__ err, uint32_t* __restrict__ qweight,
                                                           uint32_t* __restrict__ qzeros,
                                                           uint16_t* __restrict__ scales) {
    __shared__ float su[kBlock * kBlock];
    const int lane = threadIdx.x;
    // the block's piece of the factor, rows and columns [c0, c0 + n_cols): the diagonal and what lies
    // right of it (16-B pieces; a piece wholly left of the diagonal is never read), zeros past n_cols
#pragma unroll 4
    for (int idx = lane; idx < kBlock * kBlock / 4; idx += 64) {
        const int r = idx / (kBlock / 4), c4 = 4 * (idx % (kBlock / 4));
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r < n_cols && c4 < n_cols && c4 + 3 >= r) v = *(const float4*)(u + (c0 + r) * K + c0 + c4);
        ((float4*)su)[idx] = v;
    }
    __syncthreads();

    const int64_t row = (int64_t)blockIdx.x * 64 + lane;
    const bool live = row < N;
    float* wr = work + (live ? row : 0) * K + c0;
    f2 w[kBlock / 2];
#pragma unroll
    for (int c = 0; c < kBlock / 4; ++c) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (live && 4 * c < n_cols) v = ((const float4*)wr)[c];
        w[2 * c] = f2{v.x, v.y};
        w[2 * c + 1] = f2{v.z, v.w};
    }
    RoundState st;
    st.s = 0.0f;
    st.z = 0.0f;
    st.acc = 0u;
    st.e[0] = st.e[1] = st.e[2] = st.e[3] = 0.0f;
    round_chunk<0>(w, st, m, su, live, row, K, c0, n_cols, err, qweight, qzeros, scales);
    if (n_cols > kStep) round_chunk<1>(w, st, m, su, live, row, K, c0, n_cols, err, qweight, qzeros, scales);
    if (n_cols > 2 * kStep) round_chunk<2>(w, st, m, su, live, row, K, c0, n_cols, err, qweight, qzeros, scales);
    if (n_cols > 3 * kStep) round_chunk<3>(w, st, m, su, live, row, K, c0, n_cols, err, qweight, qzeros, scales);
#pragma unroll
    for (int c = 0; c < kBlock / 4; ++c)
        if (live && 4 * c < n_cols) ((float4*)wr)[c] = make_float4(w[2 * c].x, w[2 * c].y, w[2 * c + 1].x, w[2 * c + 1].y);
}

}  // namespace
}  // namespace awq

extern "C" int awq_gptq_round_block(float* work, int64_t N, int64_t K, int64_t group_size, int bits, int symmetric,
                                    const float* u, int64_t col_begin, int64_t n_cols, float* err, int32_t* qweight,
                                    int32_t* qzeros, uint16_t* scales, void* stream) {
    using namespace awq;
    set_error(AWQ_OK, "");
    if (N < 0 || K < 0 || col_begin < 0 || n_cols < 0)
        return fail(AWQ_EINVAL, "negative size (N=%lld, K=%lld, col_begin=%lld, n_cols=%lld)", (long long)N, (long long)K,
                    (long long)col_begin, (long long)n_cols);
    if (bits != 4 && bits != 8) return fail(AWQ_EUNSUPPORTED, "Unsupported bit width: %d. Supported: 4, 8.", bits);
    if (symmetric != 0 && symmetric != 1) return fail(AWQ_EINVAL, "symmetric must be 0 or 1: %d", symmetric);
    if (group_size != 32 && group_size != 64 && group_size != 128)
        return fail(AWQ_EUNSUPPORTED, "awq_gptq_round_block takes group_size 32, 64 or 128: %lld", (long long)group_size);
    if (K % group_size != 0)
        return fail(AWQ_EINVAL, "in_features must be a multiple of group_size (K=%lld, group_size=%lld)", (long long)K,
                    (long long)group_size);
    if (n_cols > kBlock || n_cols % group_size != 0)
        return fail(AWQ_EINVAL, "n_cols must be a multiple of group_size and at most %d (n_cols=%lld, group_size=%lld)",
                    kBlock, (long long)n_cols, (long long)group_size);
    if (col_begin % group_size != 0 || col_begin % 8 != 0 || col_begin > K || n_cols > K - col_begin)
        return fail(AWQ_EINVAL, "col_begin must be a multiple of group_size and of 8 with col_begin + n_cols <= K "
                                "(col_begin=%lld, n_cols=%lld, K=%lld)", (long long)col_begin, (long long)n_cols,
                    (long long)K);
    if (N == 0 || K == 0 || n_cols == 0) return AWQ_OK;
    if (N > (int64_t)0x7FFFFFFF || K > (int64_t)0x7FFFFFFF)
        return fail(AWQ_EUNSUPPORTED, "awq_gptq_round_block: N and K are limited to 2^31 - 1 (N=%lld, K=%lld)",
                    (long long)N, (long long)K);
    if (!work || !u || !err || !qweight || !qzeros || !scales)
        return fail(AWQ_EINVAL, "null argument: work, u, err, qweight, qzeros and scales are all needed");
    if (!aligned(work, 16) || !aligned(u, 16) || !aligned(err, 16) || !aligned(qweight, 4) || !aligned(qzeros, 4) ||
        !aligned(scales, 2))
        return fail(AWQ_EINVAL, "awq_gptq_round_block: work, u and err must be 16-B aligned, qweight and qzeros 4-B, "
                                "scales 2-B");
    RoundMode m;
    m.gs = (int)group_size;
    m.bits = bits;
    m.sym = symmetric;
    m.qmin_i = symmetric ? -(1 << (bits - 1)) : 0;
    m.qmin = (float)m.qmin_i;
    m.qmax = (float)(m.qmin_i + (1 << bits) - 1);
    m.nan_field = (uint32_t)(0u - (uint32_t)m.qmin_i) & ((1u << bits) - 1u);
    m.nan_code = nan_scale_code(AWQ_DTYPE_F32, symmetric, false);
    hipLaunchKernelGGL(awq_gptq_round_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, work, N, K,
                       m, u, col_begin, (int)n_cols, err, (uint32_t*)qweight, (uint32_t*)qzeros, scales);
    return hip_status(hipPeekAtLastError(), "awq gptq round kernel");
}
