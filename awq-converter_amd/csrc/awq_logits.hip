// awq_logits.hip — the evaluation tail's memory-bound op (include/awq_hip.h awq_logit_compare): two
// logit matrices [T, V] in, per row the negative log-likelihood of a target under each, the KL
// divergence between their softmaxes and both argmaxes out.  One pass over each matrix in its
// storage dtype, fp32 arithmetic, no scratch buffer, no atomics.
//
// Structure.  One 256-thread workgroup owns a row (rows beyond the grid in later loop trips).  The
// row is cut into 8-element chunks c = 0 .. ceil(V / 8) - 1; thread i takes chunks i, i + 256,
// i + 512, ... in ascending order and carries an online-softmax state per matrix,
//   m (running max), S = sum exp(x - m), for ref also A = sum exp(a - m) (a - b),
// rescaled by exp(m_old - m_new) whenever a chunk raises m (raise_max, add_chunk).  After the chain the
// workgroup takes the row maximum M (order-free), every thread rescales its state to M once, and
// the sums are added in one fixed tree: awq_lanes.h wave_sum over a wave's 64 threads, then
// (w0 + w1) + (w2 + w3) over the four waves.  The argmax is the lowest index among the threads
// whose m equals M; every thread keeps the first index that reached its own m.
// ref and q go through the same functions (raise_max, add_chunk, the same tree), so bit-identical rows give
// bit-identical m, S and lse, and kl = (A / S_r - lse_r) + lse_q = +0 exactly.
//
// Paths.  VEC: 16-B loads for every chunk that lies wholly inside [0, V) (16-B aligned bases, row
// strides a multiple of 8 elements, 4 for fp32); the ragged last chunk, and every chunk of the
// element-aligned path, is loaded element by element under its bound.  The chunk-to-thread map,
// the arithmetic on a chunk and the tree are one body, so both paths give the same bits.
#include "awq_quant.h"

namespace awq {
namespace {

constexpr int kThreads = 256;          // one row per workgroup
constexpr int kWaves = kThreads / 64;
constexpr unsigned kMaxGrid = 65536;   // rows beyond it: later trips of the row loop

struct CompareArgs {
    const void* ref;
    const void* q;
    const int64_t* targets;
    float* nll_ref;
    float* nll_q;
    float* kl;
    int32_t* argmax_ref;
    int32_t* argmax_q;
    int64_t T, V, ref_stride, q_stride;
};

// chunk c of a row: elements 8 c .. 8 c + 7 as fp32; past V: +0 (the caller masks them by index)
template <typename F, bool VEC>
__device__ __forceinline__ void load_chunk(const void* base, int64_t row0, int64_t c, int64_t V, float (&v)[8]) {
    if (VEC && 8 * c + 8 <= V) {
        load8<F>(base, row0 + 8 * c, v);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (8 * c + j < V) ? load1<F>(base, row0 + 8 * c + j) : 0.0f;
    }
}

// one thread's online-softmax state of one matrix
struct RowState {
    float m, S;
    int32_t idx;
    int bad;
};

__device__ __forceinline__ RowState state_init() { return RowState{-__builtin_inff(), 0.0f, INT32_MAX, 0}; }

// the chunk's maximum over its n valid elements, and whether any of them is NaN / +-inf
__device__ __forceinline__ float chunk_max(const float (&v)[8], int n, int& bad) {
    float cm = -__builtin_inff();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j < n) {
            bad |= !__builtin_isfinite(v[j]);
            cm = __builtin_fmaxf(cm, v[j]);
        }
    }
    return cm;
}

// raise the state's m to the chunk's maximum; returns the factor the sums take, exp(m_old - m_new)
// (exactly 1 when m stays).  The first index attaining a new m is the chunk's lowest such element.
__device__ __forceinline__ float raise_max(RowState& st, const float (&v)[8], int n, float cm, int64_t c) {
    float e = 1.0f;
    if (cm > st.m) {
        e = expf(st.m - cm);
        st.m = cm;
        int first = 7;
#pragma unroll
        for (int j = 6; j >= 0; --j) first = (j < n && v[j] == cm) ? j : first;
        st.idx = (int32_t)(8 * c + first);
    }
    return e;
}

// w[j] = exp(v[j] - m) for the valid elements (+0 past n); S = S e + (((0 + w0) + w1) + ... + w7)
__device__ __forceinline__ void add_chunk(RowState& st, const float (&v)[8], int n, float e, float (&w)[8]) {
    float cs = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        w[j] = (j < n) ? expf(v[j] - st.m) : 0.0f;
        cs += w[j];
    }
    st.S = st.S * e + cs;
}

// the workgroup's reductions: wave first (awq_lanes.h), then the four waves' values in a fixed order
struct BlockShared {
    float mr[kWaves], mq[kWaves], Sr[kWaves], Sq[kWaves], A[kWaves];
    int32_t ir[kWaves], iq[kWaves];
    int bad[kWaves];
};

template <typename F, bool VEC, bool HASQ>
__global__ __launch_bounds__(kThreads) void logit_compare_kernel(CompareArgs p) {
    __shared__ BlockShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t V = p.V, nchunk = (V + 7) / 8;
    for (int64_t t = blockIdx.x; t < p.T; t += gridDim.x) {
        const int64_t ra = t * p.ref_stride, rq = HASQ ? t * p.q_stride : 0;
        RowState sr = state_init(), sq = state_init();
        float A = 0.0f;
#pragma unroll 2
        for (int64_t c = tid; c < nchunk; c += kThreads) {
            const int n = (int)((V - 8 * c < 8) ? V - 8 * c : 8);
            float a[8], b[8], w[8];
            load_chunk<F, VEC>(p.ref, ra, c, V, a);
            if (HASQ) load_chunk<F, VEC>(p.q, rq, c, V, b);
            const float er = raise_max(sr, a, n, chunk_max(a, n, sr.bad), c);
            add_chunk(sr, a, n, er, w);
            if (HASQ) {
                float ca = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) ca += w[j] * ((j < n) ? a[j] - b[j] : 0.0f);
                A = A * er + ca;
                float wq[8];
                const float eq = raise_max(sq, b, n, chunk_max(b, n, sq.bad), c);
                add_chunk(sq, b, n, eq, wq);
            }
        }
        // the row maxima and the non-finite flags (order-free)
        const float wmr = wave_max(sr.m), wmq = HASQ ? wave_max(sq.m) : 0.0f;
        const int wbad = wave_or(sr.bad | (sq.bad << 1));
        if (lane == 0) {
            sh.mr[wave] = wmr;
            sh.mq[wave] = wmq;
            sh.bad[wave] = wbad;
        }
        __syncthreads();
        const float Mr = __builtin_fmaxf(__builtin_fmaxf(sh.mr[0], sh.mr[1]), __builtin_fmaxf(sh.mr[2], sh.mr[3]));
        const float Mq = __builtin_fmaxf(__builtin_fmaxf(sh.mq[0], sh.mq[1]), __builtin_fmaxf(sh.mq[2], sh.mq[3]));
        const int bad = sh.bad[0] | sh.bad[1] | sh.bad[2] | sh.bad[3];
        // every thread's sums to the row maximum (a thread at the maximum keeps its bits; one
        // without a chunk holds m = -inf and +0 sums, and exp(-inf) = +0), then the tree
        const float fr = (sr.m == Mr) ? 1.0f : expf(sr.m - Mr);
        const float fq = (!HASQ || sq.m == Mq) ? 1.0f : expf(sq.m - Mq);
        const float wSr = wave_sum(sr.S * fr);
        const float wA = HASQ ? wave_sum(A * fr) : 0.0f;
        const float wSq = HASQ ? wave_sum(sq.S * fq) : 0.0f;
        const int32_t wir = wave_min((sr.m == Mr) ? sr.idx : INT32_MAX);
        const int32_t wiq = HASQ ? wave_min((sq.m == Mq) ? sq.idx : INT32_MAX) : 0;
        if (lane == 0) {
            sh.Sr[wave] = wSr;
            sh.A[wave] = wA;
            sh.Sq[wave] = wSq;
            sh.ir[wave] = wir;
            sh.iq[wave] = wiq;
        }
        __syncthreads();
        if (tid == 0) {
            const float nan = __builtin_nanf("");
            const bool bad_r = bad & 1, bad_q = bad & 2;
            const float Sr = (sh.Sr[0] + sh.Sr[1]) + (sh.Sr[2] + sh.Sr[3]);
            const float lse_r = Mr + logf(Sr);
            float Sq = 1.0f, lse_q = 0.0f;
            if (HASQ) {
                Sq = (sh.Sq[0] + sh.Sq[1]) + (sh.Sq[2] + sh.Sq[3]);
                lse_q = Mq + logf(Sq);
            }
            if (p.targets) {
                const int64_t g = p.targets[t];
                float nr = 0.0f, nq = 0.0f;
                if (g >= V) {
                    nr = nq = nan;
                } else if (g >= 0) {
                    nr = bad_r ? nan : lse_r - load1<F>(p.ref, ra + g);
                    if (HASQ) nq = bad_q ? nan : lse_q - load1<F>(p.q, rq + g);
                }
                if (p.nll_ref) p.nll_ref[t] = nr;
                if (HASQ && p.nll_q) p.nll_q[t] = nq;
            }
            if (p.argmax_ref) p.argmax_ref[t] = bad_r ? -1 : min(min(sh.ir[0], sh.ir[1]), min(sh.ir[2], sh.ir[3]));
            if (HASQ) {
                if (p.argmax_q) p.argmax_q[t] = bad_q ? -1 : min(min(sh.iq[0], sh.iq[1]), min(sh.iq[2], sh.iq[3]));
                if (p.kl) {
                    const float Asum = (sh.A[0] + sh.A[1]) + (sh.A[2] + sh.A[3]);
                    p.kl[t] = (bad_r || bad_q) ? nan : (Asum / Sr - lse_r) + lse_q;
                }
            }
        }
        // the next row's first barrier orders its second-phase writes behind these reads; its
        // first-phase writes follow this row's second barrier, past every first-phase read
    }
}

template <typename F>
hipError_t launch_compare(const CompareArgs& p, bool vec, hipStream_t stream) {
    const unsigned grid = diag_cap((unsigned)(p.T < (int64_t)kMaxGrid ? p.T : (int64_t)kMaxGrid));
    if (p.q) {
        if (vec) hipLaunchKernelGGL((logit_compare_kernel<F, true, true>), dim3(grid), dim3(kThreads), 0, stream, p);
        else hipLaunchKernelGGL((logit_compare_kernel<F, false, true>), dim3(grid), dim3(kThreads), 0, stream, p);
    } else {
        if (vec) hipLaunchKernelGGL((logit_compare_kernel<F, true, false>), dim3(grid), dim3(kThreads), 0, stream, p);
        else hipLaunchKernelGGL((logit_compare_kernel<F, false, false>), dim3(grid), dim3(kThreads), 0, stream, p);
    }
    return hipPeekAtLastError();
}

hipError_t run_compare(int dtype, const CompareArgs& p, bool vec, hipStream_t s) {
    switch (dtype) {
    case AWQ_DTYPE_BF16: return launch_compare<FmtBF16>(p, vec, s);
    case AWQ_DTYPE_F16: return launch_compare<FmtF16>(p, vec, s);
    default: return launch_compare<FmtF32>(p, vec, s);
    }
}

}  // namespace
}  // namespace awq

using awq::aligned;
using awq::fail;

extern "C" {

int awq_logit_compare(const void* ref, const void* q, int dtype, int64_t T, int64_t V, int64_t ref_row_stride,
                      int64_t q_row_stride, const int64_t* targets, float* nll_ref, float* nll_q, float* kl,
                      int32_t* argmax_ref, int32_t* argmax_q, void* stream) {
    awq::set_error(AWQ_OK, "");
    if (dtype != AWQ_DTYPE_BF16 && dtype != AWQ_DTYPE_F16 && dtype != AWQ_DTYPE_F32)
        return fail(AWQ_EUNSUPPORTED, "awq_logit_compare takes bf16 / fp16 / fp32 logits (dtype code %d)", dtype);
    if (T < 0 || V < 1)
        return fail(AWQ_EINVAL, "awq_logit_compare: T (%lld) must be >= 0 and V (%lld) >= 1", (long long)T, (long long)V);
    if (T == 0) return AWQ_OK;
    if (V >= ((int64_t)1 << 31)) return fail(AWQ_EINVAL, "awq_logit_compare: V (%lld) must be below 2^31", (long long)V);
    if (!ref) return fail(AWQ_EINVAL, "awq_logit_compare: ref is NULL");
    if (!q) q_row_stride = V;
    if (ref_row_stride < V || q_row_stride < V)
        return fail(AWQ_EINVAL, "awq_logit_compare: a row stride (ref %lld, q %lld) smaller than V (%lld)",
                    (long long)ref_row_stride, (long long)q_row_stride, (long long)V);
    const int64_t lim = (int64_t)1 << 60;
    if (T > lim / ref_row_stride || T > lim / q_row_stride)
        return fail(AWQ_EINVAL, "awq_logit_compare: T x row stride above 2^60 (T=%lld, strides %lld, %lld)", (long long)T,
                    (long long)ref_row_stride, (long long)q_row_stride);
    const int64_t sm = dtype == AWQ_DTYPE_F32 ? 4 : 8;
    const bool vec = aligned(ref, 16) && ref_row_stride % sm == 0 && (!q || (aligned(q, 16) && q_row_stride % sm == 0));
    awq::CompareArgs p{ref, q, targets, nll_ref, nll_q, kl, argmax_ref, argmax_q, T, V, ref_row_stride, q_row_stride};
    return awq::hip_status(awq::run_compare(dtype, p, vec, (hipStream_t)stream), "awq logit compare");
}

}  // extern "C"
