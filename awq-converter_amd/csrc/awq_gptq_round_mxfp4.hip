// awq_gptq_round_mxfp4.hip — GPTQ error-compensated rounding of one block of input columns onto the
// MXFP4 grid (include/awq_hip.h awq_gptq_round_block_mxfp4).
//
// The chain is awq_gptq_round.hip's: column c of a row is rounded, its error e over the factor's
// diagonal is taken off every later column of the call through row c of the factor, and only then
// can column c + 1 be rounded.  What differs is the grid (a power-of-two scale per fixed block of 32,
// the E2M1 magnitudes) and with it the balance: an element is rounded by ONE fp32 addition
// (awq_mxfp4.hip), so the chain is short and the update of the later columns is what a lane spends
// its time on.  Hence a finer split than the integer kernel's lane per row:
//
//   a QUAD of lanes per row.  Lane q of the quad owns the call's columns [32 q, 32 q + 32) — one
//   MXFP4 block — in 32 VGPRs.  The block's amax, its "mse" candidates, its 32 codes (packed eight to
//   a dword in a register) and its scale byte never leave the lane.  While lane q walks its block
//   (chunk C = q of the chain), e goes to the whole quad by a DPP quad broadcast; lane q takes it off
//   its own later elements, the lanes q > C off all 32 of theirs (v_pk_mul_f32 / v_pk_add_f32 on
//   register pairs), the lanes q < C are done and sit the update out (exec).
//
//   a wave holds 16 rows; a workgroup of 1, 2 or 4 waves stages the upper triangle of the call's
//   128 x 128 piece of the factor in 64 KiB of LDS once (zeros left of the diagonal and past n_cols).
//   Row c of the tile is read as eight 16-B pieces per lane, four distinct addresses per wave (one
//   per lane of a quad), the rest broadcasts.  The owner's piece holds the diagonal U[c][c], so the
//   division needs no read of its own.  The host picks the waves per workgroup so that the grid
//   covers the device before workgroups grow: rows do not meet and a column's operations are fixed
//   by the definition, so the bits do not depend on the split.
//
// Every lane runs the owner's arithmetic on its own element (a non-owner's result is dropped: the
// broadcast takes the owner's e, the stores are the owner's), so there is no divergence on the chain
// itself.  The chain is unrolled completely: every register index is a constant.
//
// Arithmetic: every operation is a single fp32 operation rounded on its own (-ffp-contract=off, IEEE
// division), fp32 subnormals kept, so the NumPy float32 restatement tests/gptq_mxfp4_ref.py gives
// the same bits.
#include "awq_quant.h"

namespace awq {
namespace {

constexpr int kCall = 128;     // widest call: the tile's side
constexpr int kBlk = 32;       // the MXFP4 block = a lane's register window
constexpr int kPairs = kBlk / 2;
constexpr int kRowsPerWave = 16;

struct BlockState {            // per lane: its block's scale, set at the block's first column
    float inv;                 // 2^-X
    float scale;               // 2^X
    bool bad;                  // the block holds a NaN or an inf
    uint32_t acc;              // codes of the dword being filled
    float e[4];                // errors of the 16-B err store being filled
};

__device__ __forceinline__ float elem(const f2 (&w)[kPairs], int i) { return (i & 1) ? w[i >> 1].y : w[i >> 1].x; }

// one element at the scale 2^-X = inv: the one-addition rounding of awq_mxfp4.hip.  -> the code's
// magnitude index; m: the rounded magnitude; t: |x| 2^-X before the saturation
__device__ __forceinline__ uint32_t round_e2m1(float x, float inv, float& m, float& t) {
    t = __builtin_fabsf(x) * inv;
    const float v = __builtin_fminf(t, 6.0f);
    const uint32_t k = max(__float_as_uint(v) >> 23, 127u);            // 127, 128, 129
    const float magic = __uint_as_float((k + 22u) << 23);
    const float r = v + magic;                                         // the one rounding
    m = r - magic;
    return (__float_as_uint(r) & 7u) + 2u * k - 254u;
}

// sum of (t - m)^2 over the lane's 32 elements at the scale inv: four runs of 8 in order from +0,
// (p0 + p1) + (p2 + p3) — awq_quantize_mxfp4's lanes and quad tree
__device__ __forceinline__ float block_sq_error(const f2 (&w)[kPairs], float inv) {
    float p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float m, t;
            round_e2m1(elem(w, 8 * r + i), inv, m, t);
            const float d = t - m;
            s = s + d * d;
        }
        p[r] = s;
    }
    return (p[0] + p[1]) + (p[2] + p[3]);
}

// the block's scale from its 32 working values as they stand: awq_quantize_mxfp4's rule for fp32 input
__device__ __forceinline__ uint32_t block_scale(const f2 (&w)[kPairs], int rule, BlockState& st) {
    uint32_t amax = 0u;
#pragma unroll
    for (int i = 0; i < kBlk; ++i) amax = max(amax, __float_as_uint(elem(w, i)) & 0x7FFFFFFFu);
    st.bad = amax >= 0x7F800000u;
    const float af = __uint_as_float(amax);
    uint32_t e = amax == 0u ? 127u : max(amax >> 23, 2u) - 2u;
    const float inv = __uint_as_float((254u - e) << 23);               // 2^-X, e <= 252
    bool up = false;
    if (rule == AWQ_MXFP4_MSE) up = 4.0f * block_sq_error(w, inv * 0.5f) < block_sq_error(w, inv);
    else if (rule == AWQ_MXFP4_CEIL) up = af * inv > 6.0f;
    e += up ? 1u : 0u;
    st.inv = up ? inv * 0.5f : inv;
    st.scale = __uint_as_float(max(e << 23, 0x00400000u));             // e = 0: the subnormal 2^-127
    return st.bad ? 255u : e;
}

// column I of chunk C: the call's column 32 C + I, owned by lane q == C of every quad
template <int C, int I>
__device__ __forceinline__ void round_step(f2 (&w)[kPairs], BlockState& st, const float* su, int q, bool live,
                                           float* err_row, uint32_t* code_row) {
    // row 32 C + I of the tile, this lane's 32 columns
    const float* ur = su + (C * kBlk + I) * kCall + q * kBlk;
    f2 ub[kPairs];
#pragma unroll
    for (int k = 0; k < kBlk / 4; ++k) {
        const float4 v = *(const float4*)(ur + 4 * k);
        ub[2 * k] = f2{v.x, v.y};
        ub[2 * k + 1] = f2{v.z, v.w};
    }
    const float wi = elem(w, I);
    float m, t;
    const uint32_t mag = round_e2m1(wi, st.inv, m, t);
    const uint32_t sign = __float_as_uint(wi) & 0x80000000u;
    const float dq = __uint_as_float(__float_as_uint(m * st.scale) | sign);   // exact
    const float d = wi - dq;
    float e = d / elem(ub, I);                                                // the owner's piece: U[c][c]
    if (st.bad || !(__builtin_isfinite(wi) && __builtin_isfinite(dq) && __builtin_isfinite(e))) e = 0.0f;
    const uint32_t code = st.bad ? 0u : (mag | (sign >> 28));
    st.acc = (I & 7) ? st.acc | (code << (4 * (I & 7))) : code;
    e = dpp_mov<C * 0x55>(e);                                                 // quad_perm [C, C, C, C]
    st.e[I & 3] = e;
    if (q == C && live) {
        if ((I & 7) == 7) code_row[(C * kBlk + I) >> 3] = st.acc;
        if ((I & 3) == 3) *(float4*)(err_row + C * kBlk + I - 3) = make_float4(st.e[0], st.e[1], st.e[2], st.e[3]);
    }
    // take e U[c][j] off every later column j: product and difference rounded separately
    const f2 ev = {e, e};
    if (q >= C) {                  // the owner's later elements and every later lane's same positions
        if ((I & 1) == 0) w[I >> 1].y = w[I >> 1].y - e * ub[I >> 1].y;
#pragma unroll
        for (int p = (I >> 1) + 1; p < kPairs; ++p) w[p] = pk_add(w[p], -pk_mul(ev, ub[p]));
    }
    if (q > C) {                   // the later lanes' positions up to I
#pragma unroll
        for (int p = 0; p < (I >> 1); ++p) w[p] = pk_add(w[p], -pk_mul(ev, ub[p]));
        if (I & 1) w[I >> 1] = pk_add(w[I >> 1], -pk_mul(ev, ub[I >> 1]));
        else w[I >> 1].x = w[I >> 1].x - e * ub[I >> 1].x;
    }
    // every column is up to date before the next step begins, and no read of a later step's row
    // moves up into this one: left alone the compiler hoists the reads of many steps and spills
#pragma unroll
    for (int p = 0; p < kPairs; ++p) asm volatile("" : "+v"(w[p]));
    __builtin_amdgcn_sched_barrier(0);
}

template <int C, int I>
__device__ __forceinline__ void round_steps(f2 (&w)[kPairs], BlockState& st, const float* su, int q, bool live,
                                            float* err_row, uint32_t* code_row) {
    if constexpr (I < kBlk) {
        round_step<C, I>(w, st, su, q, live, err_row, code_row);
        round_steps<C, I + 1>(w, st, su, q, live, err_row, code_row);
    }
}

template <int C>
__device__ __forceinline__ void round_chunk(f2 (&w)[kPairs], BlockState& st, int rule, const float* su, int q, bool live,
                                            float* err_row, uint32_t* code_row, uint8_t* scale_row) {
    const uint32_t e = block_scale(w, rule, st);       // every lane on its own values; the owner's is the block's
    if (q == C && live) scale_row[C] = (uint8_t)e;
    round_steps<C, 0>(w, st, su, q, live, err_row, code_row);
}

__global__ __launch_bounds__(256) void awq_gptq_round_mxfp4_kernel(float* __restrict__ work, int64_t N, int64_t K, int rule,
                                                                  const float* __restrict__ u, int64_t c0, int n_cols,
                                                                  float* __restrict__ err, uint8_t* __restrict__ codes,
                                                                  uint8_t* __restrict__ scales) {
    __shared__ float su[kCall * kCall];
    const int tid = threadIdx.x, nthr = blockDim.x;
    // the call's piece of the factor, rows and columns [c0, c0 + n_cols): the diagonal and what lies
    // right of it in 16-B pieces, zeros everywhere else
    for (int idx = tid; idx < kCall * kCall / 4; idx += nthr) {
        const int r = idx / (kCall / 4), c4 = 4 * (idx % (kCall / 4));
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r < n_cols && c4 < n_cols && c4 + 3 >= r) v = *(const float4*)(u + (c0 + r) * K + c0 + c4);
        ((float4*)su)[idx] = v;
    }
    __syncthreads();

    const int q = tid & 3;
    const int64_t row = (int64_t)blockIdx.x * (nthr >> 2) + (tid >> 2);
    const int nch = n_cols / kBlk;                     // chunks of the call
    const bool live = row < N;
    const bool mine = live && q < nch;                 // this lane's block is part of the call
    const int64_t r0 = live ? row : 0;
    float* wr = work + r0 * K + c0 + (mine ? q : 0) * kBlk;
    f2 w[kPairs];
#pragma unroll
    for (int k = 0; k < kBlk / 4; ++k) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (mine) v = ((const float4*)wr)[k];
        w[2 * k] = f2{v.x, v.y};
        w[2 * k + 1] = f2{v.z, v.w};
    }
    float* err_row = err + r0 * n_cols;
    uint32_t* code_row = (uint32_t*)(codes + r0 * (K / 2) + c0 / 2);
    uint8_t* scale_row = scales + r0 * (K / kBlk) + c0 / kBlk;
    BlockState st;
    st.inv = st.scale = 1.0f;
    st.bad = false;
    st.acc = 0u;
    st.e[0] = st.e[1] = st.e[2] = st.e[3] = 0.0f;
    round_chunk<0>(w, st, rule, su, q, live, err_row, code_row, scale_row);
    if (nch > 1) round_chunk<1>(w, st, rule, su, q, live, err_row, code_row, scale_row);
    if (nch > 2) round_chunk<2>(w, st, rule, su, q, live, err_row, code_row, scale_row);
    if (nch > 3) round_chunk<3>(w, st, rule, su, q, live, err_row, code_row, scale_row);
#pragma unroll
    for (int k = 0; k < kBlk / 4; ++k)
        if (mine) ((float4*)wr)[k] = make_float4(w[2 * k].x, w[2 * k].y, w[2 * k + 1].x, w[2 * k + 1].y);
}

}  // namespace
}  // namespace awq

extern "C" int awq_gptq_round_block_mxfp4(float* work, int64_t N, int64_t K, int rule, const float* u, int64_t col_begin,
                                          int64_t n_cols, float* err, uint8_t* codes, uint8_t* scales, void* stream) {
    using namespace awq;
    set_error(AWQ_OK, "");
    const char* me = "awq_gptq_round_block_mxfp4";
    if (N < 0 || K < 0 || col_begin < 0 || n_cols < 0)
        return fail(AWQ_EINVAL, "%s: negative size (N=%lld, K=%lld, col_begin=%lld, n_cols=%lld)", me, (long long)N,
                    (long long)K, (long long)col_begin, (long long)n_cols);
    if (rule != AWQ_MXFP4_FLOOR && rule != AWQ_MXFP4_CEIL && rule != AWQ_MXFP4_MSE)
        return fail(AWQ_EINVAL, "%s: scale rule %d is not floor (0), ceil (1) or mse (2)", me, rule);
    if (K % kBlk != 0) return fail(AWQ_EINVAL, "%s: K %% 32 must be 0, the MXFP4 block (K=%lld)", me, (long long)K);
    if (n_cols > kCall || n_cols % kBlk != 0)
        return fail(AWQ_EINVAL, "%s: n_cols must be a multiple of 32 and at most %d (n_cols=%lld)", me, kCall,
                    (long long)n_cols);
    if (col_begin % kBlk != 0 || col_begin > K || n_cols > K - col_begin)
        return fail(AWQ_EINVAL, "%s: col_begin must be a multiple of 32 with col_begin + n_cols <= K (col_begin=%lld, "
                                "n_cols=%lld, K=%lld)", me, (long long)col_begin, (long long)n_cols, (long long)K);
    if (N == 0 || K == 0 || n_cols == 0) return AWQ_OK;
    if (N > (int64_t)0x7FFFFFFF || K > (int64_t)0x7FFFFFFF)
        return fail(AWQ_EUNSUPPORTED, "%s: N and K are limited to 2^31 - 1 (N=%lld, K=%lld)", me, (long long)N, (long long)K);
    if (!work || !u || !err || !codes || !scales)
        return fail(AWQ_EINVAL, "%s: null argument: work, u, err, codes and scales are all needed", me);
    if (!aligned(work, 16) || !aligned(u, 16) || !aligned(err, 16) || !aligned(codes, 4))
        return fail(AWQ_EINVAL, "%s: work, u and err must be 16-B aligned, codes 4-B", me);
    // waves per workgroup: one until a wave per workgroup covers the device's 256 CUs, then two, then four
    // (more rows per staged tile); the bits do not depend on it
    const int waves = N >= 4 * kRowsPerWave * 256 ? 4 : N >= 2 * kRowsPerWave * 256 ? 2 : 1;
    const int64_t rows_per_wg = (int64_t)waves * kRowsPerWave;
    hipLaunchKernelGGL(awq_gptq_round_mxfp4_kernel, dim3((unsigned)((N + rows_per_wg - 1) / rows_per_wg)), dim3(64 * waves),
                       0, (hipStream_t)stream, work, N, K, rule, u, col_begin, (int)n_cols, err, codes, scales);
    return hip_status(hipPeekAtLastError(), "awq gptq round mxfp4 kernel");
}
