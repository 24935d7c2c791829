// awq_calib.hip — the calibration pass' memory-bound ops (include/awq_hip.h awq_act_stats_accum,
// awq_rmsnorm_stats, awq_swiglu_stats): every linear of a decoder block reads the output of an
// RMSNorm, of the attention, or of a SwiGLU product; these entries produce that output (the norm
// and the product) and add its column statistics sum |v| and sum v^2 to fp64 running sums in
// awq_act_stats' canonical order, so the sums of many micro-batches are the bits of awq_act_stats
// on the concatenated rows.
//
// Structure.  One tile kernel for the three entries (calib_tile_kernel): a workgroup takes one
// 256-row block x 32 columns, as colsum_tile_kernel (awq_actsearch.hip) does: every thread loads
// 8-column octets of four rows (16-B loads, all in flight at once), forms the output values
// (PROD: the input itself / w * RN_D(x * r_t) / RN_D(silu(g)) * u), stores them (16-B stores) and
// puts them in LDS as fp32; then 256 lanes run one 32-row sub-block chain each (rows ascending,
// fp64) and 32 lanes add the block's sub-block sums in order -> work[block][k].  A second, small
// kernel (acc_add_kernel) adds the blocks' sums, ascending, onto the running sums: block sums
// added ascending onto a running value that started at +0 is the sum colmean_kernel forms.  The
// order across workgroups is thereby fixed without atomics.  The norm's row reduction is a kernel
// of its own before the tile kernel (rms_rows_kernel, one wave per row -> r_t in the workspace);
// the tile kernel's read of x is the second one (a micro-batch sits in the Infinity Cache).
// Anything the 16-B path cannot take (K % 8 != 0, a row stride that is no multiple of 8,
// element-aligned pointers): calib_col_kernel, one lane per column and block, the same chains.
//
// The chain arithmetic restates colsum_tile_kernel / colsum_kernel (MODE 0) term by term; the
// GPU tests pin the bits of all paths against awq_act_stats and the oracle.
#include <string>

#include "awq_quant.h"

namespace awq {
namespace {

constexpr int kRowBlock = 256;   // rows per column-sum block   (awq_act_stats' canonical order)
constexpr int kRowSub = 32;      // rows per sub-block
constexpr int kColTile = 32;     // columns per workgroup of the tile kernel

enum { PROD_PLAIN = 0, PROD_NORM = 1, PROD_SWIGLU = 2 };

struct ProdArgs {
    const void* a;      // x (plain, norm) / gate
    const void* b;      // norm weight [K] / up
    const float* r;     // norm: r_t fp32 [rows]
    void* out;          // [rows, K] contiguous (norm, swiglu)
    int64_t sa, sb;     // row strides of a and of up, in elements
};

// RN_D of an fp32 value the optimizer cannot see through (the op before it stays an fp32 op)
template <typename F>
__device__ __forceinline__ float rnd(float a) {
    return F::rn(opaque(a));
}

template <typename F>
__device__ __forceinline__ uint32_t dtype_bits(float y) {   // y: a value of the dtype
    if constexpr (F::NW == 2) return __float_as_uint(y);
    else if constexpr (std::is_same<F, FmtF16>::value) return __builtin_bit_cast(uint16_t, (_Float16)y);
    else return __float_as_uint(y) >> 16;
}

template <typename F>
__device__ __forceinline__ void store1(void* base, int64_t i, float y) {
    if constexpr (F::NW == 2) ((float*)base)[i] = y;
    else ((uint16_t*)base)[i] = (uint16_t)dtype_bits<F>(y);
}

template <typename F>
__device__ __forceinline__ void store8(void* base, int64_t i, const float (&y)[8]) {
    if constexpr (F::NW == 2) {
        float4* p = (float4*)((float*)base + i);
        p[0] = make_float4(y[0], y[1], y[2], y[3]);
        p[1] = make_float4(y[4], y[5], y[6], y[7]);
    } else {
        uint32_t b[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = dtype_bits<F>(y[j]);
        *(uint4*)((uint16_t*)base + i) =
            make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
    }
}

// transformers' LlamaRMSNorm tail: weight * (x.float() * r).to(D), the product rounded into D
template <typename F>
__device__ __forceinline__ float norm_value(float x, float r, float w) {
    const float h = rnd<F>(x * r);
    return rnd<F>(w * h);
}

// RN_D(RN_D(silu(g)) * u), silu(g) = g / (1 + exp(-g)) in fp32
template <typename F>
__device__ __forceinline__ float swiglu_value(float g, float u) {
    const float e = expf(-g);
    const float s = rnd<F>(g / (1.0f + e));
    return rnd<F>(s * u);
}

// ---- the norm's row reduction: v_t = sum_k RN_f32(x^2) in fp32, r_t = 1 / sqrt(v_t / H + eps) ----
// One wave per row.  The row is cut into 8-element chunks c = 0 .. ceil(H / 8) - 1, each summed in
// order from +0 (elements past H add nothing); lane l adds the sums of chunks l, l + 64, l + 128,
// ... in ascending order from +0 (its slot); the row's sum is the pairwise tree over the 64 slots,
// adjacent pairs first (wave_sum).
template <typename F, bool VEC>
__global__ __launch_bounds__(256) void rms_rows_kernel(const void* __restrict__ x, int64_t rows, int64_t H,
                                                       float eps, float* __restrict__ r) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform
    if (t >= rows) return;
    const int64_t nchunk = (H + 7) / 8;
    float slot = 0.0f;
#pragma unroll 4
    for (int64_t c = lane; c < nchunk; c += 64) {
        float v[8];
        if (VEC) {
            load8<F>(x, t * H + 8 * c, v);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (8 * c + j < H) ? load1<F>(x, t * H + 8 * c + j) : 0.0f;
        }
        float cs = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) cs += v[j] * v[j];   // a zero term leaves a sum of squares unchanged
        slot += cs;
    }
    const float tot = wave_sum(slot);
    const float m = tot / (float)H + eps;
    const float q = __builtin_sqrtf(m);
    if (lane == 0) r[t] = 1.0f / q;
}

// ---- the tile kernel (16-B path) ----
template <typename F, int PROD, bool STATS>
__global__ __launch_bounds__(256) void calib_tile_kernel(ProdArgs p, int64_t rows, int64_t K,
                                                         double* __restrict__ part0, double* __restrict__ part1) {
    __shared__ __attribute__((aligned(16))) float sv[STATS ? kRowBlock : 1][kColTile];
    const int tid = threadIdx.x;
    const int64_t kt = (int64_t)blockIdx.x * kColTile;
    const int64_t b = blockIdx.y, r0 = b * kRowBlock;
    const int nr = (int)((r0 + kRowBlock < rows) ? kRowBlock : rows - r0);
    constexpr int OPR = kColTile / 8, RPP = 256 / OPR;   // octets per row, rows per pass
    const int oc = tid % OPR, rl = tid / OPR;           // column octet, first row
    const int64_t k0 = kt + 8 * oc;
    const bool kin = k0 < K;                            // K % 8 == 0: the octet is inside the row
    constexpr int NI = kRowBlock / RPP;
    float va[NI][8];
    float vb[PROD == PROD_SWIGLU ? NI : 1][8];
    float rr_t[NI];
    if (PROD == PROD_NORM) {
        if (kin) load8<F>(p.b, k0, vb[0]);
        else
#pragma unroll
            for (int j = 0; j < 8; ++j) vb[0][j] = 0.0f;
    }
#pragma unroll
    for (int it = 0; it < NI; ++it) {
        const int rr = rl + RPP * it;
        rr_t[it] = 0.0f;
        if (kin && rr < nr) {
            load8<F>(p.a, (r0 + rr) * p.sa + k0, va[it]);
            if (PROD == PROD_SWIGLU) load8<F>(p.b, (r0 + rr) * p.sb + k0, vb[it]);
            if (PROD == PROD_NORM) rr_t[it] = p.r[r0 + rr];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) va[it][j] = 0.0f;
            if (PROD == PROD_SWIGLU)
#pragma unroll
                for (int j = 0; j < 8; ++j) vb[it][j] = 0.0f;
        }
    }
#pragma unroll
    for (int it = 0; it < NI; ++it) {
        const int rr = rl + RPP * it;
        if (PROD != PROD_PLAIN) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (PROD == PROD_NORM) va[it][j] = norm_value<F>(va[it][j], rr_t[it], vb[0][j]);
                else va[it][j] = swiglu_value<F>(va[it][j], vb[it][j]);
            }
            if (kin && rr < nr) store8<F>(p.out, (r0 + rr) * K + k0, va[it]);
        }
        if (STATS) {
            // rows past the block's end hold what the zero inputs give; the chains below stop at nr
            *(float4*)&sv[rr][8 * oc] = make_float4(va[it][0], va[it][1], va[it][2], va[it][3]);
            *(float4*)&sv[rr][8 * oc + 4] = make_float4(va[it][4], va[it][5], va[it][6], va[it][7]);
        }
    }
    if (!STATS) return;
    __syncthreads();
    // every thread: one column of one 32-row sub-block (rows ascending, fp64); then kColTile
    // lanes add the block's sub-block sums in order
    constexpr int NSUB = kRowBlock / kRowSub;
    static_assert(NSUB * kColTile == 256, "one sub-block chain per thread");
    const int col = tid % kColTile, sub = tid / kColTile;
    const int ra = sub * kRowSub, rb = min(ra + kRowSub, nr);
    double s0 = 0.0, s1 = 0.0;
    for (int r = ra; r < rb; r += 16) {
        float t[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) t[j] = sv[(r + j < rb) ? r + j : rb - 1][col];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (r + j < rb) {
                const double d = (double)t[j];     // |v| and v * v are exact in fp64
                s0 += __builtin_fabs(d);
                s1 += d * d;
            }
        }
    }
    __shared__ double ss0[STATS ? NSUB : 1][kColTile], ss1[STATS ? NSUB : 1][kColTile];
    ss0[sub][col] = s0;
    ss1[sub][col] = s1;
    __syncthreads();
    if (tid >= kColTile || kt + tid >= K) return;
    double a0 = 0.0, a1 = 0.0;
    for (int u = 0; u < NSUB && u * kRowSub < nr; ++u) {   // non-empty sub-blocks, ascending
        a0 += ss0[u][tid];
        a1 += ss1[u][tid];
    }
    part0[b * K + kt + tid] = a0;
    part1[b * K + kt + tid] = a1;
}

// ---- any shape / alignment: one lane per column and block, the same chains ----
template <typename F, int PROD, bool STATS>
__global__ __launch_bounds__(256) void calib_col_kernel(ProdArgs p, int64_t rows, int64_t K,
                                                        double* __restrict__ part0, double* __restrict__ part1) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const int64_t b = blockIdx.y;
    const int64_t r0 = b * kRowBlock;
    const int64_t r1 = (r0 + kRowBlock < rows) ? r0 + kRowBlock : rows;
    const float w = (PROD == PROD_NORM) ? load1<F>(p.b, k) : 0.0f;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t ra = r0; ra < r1; ra += kRowSub) {
        const int64_t rb = (ra + kRowSub < r1) ? ra + kRowSub : r1;
        double u0 = 0.0, u1 = 0.0;
        for (int64_t r = ra; r < rb; ++r) {
            float v = load1<F>(p.a, r * p.sa + k);
            if (PROD == PROD_NORM) v = norm_value<F>(v, p.r[r], w);
            if (PROD == PROD_SWIGLU) v = swiglu_value<F>(v, load1<F>(p.b, r * p.sb + k));
            if (PROD != PROD_PLAIN) store1<F>(p.out, r * K + k, v);
            const double d = (double)v;
            u0 += __builtin_fabs(d);
            u1 += d * d;
        }
        s0 += u0;
        s1 += u1;
    }
    if (STATS) {
        part0[b * K + k] = s0;
        part1[b * K + k] = s1;
    }
}

// acc[k] += the blocks' sums, blocks ascending (blockIdx.y: 0 = sum |v|, 1 = sum v^2)
__global__ __launch_bounds__(256) void acc_add_kernel(const double* __restrict__ part, int64_t nblk, int64_t K,
                                                      double* __restrict__ acc0, double* __restrict__ acc1) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const double* src = part + (int64_t)blockIdx.y * nblk * K;
    double* acc = blockIdx.y ? acc1 : acc0;
    double s = acc[k];
    for (int64_t b = 0; b < nblk; ++b) s += src[b * K + k];
    acc[k] = s;
}

template <typename F, int PROD>
hipError_t launch_prod(const ProdArgs& p, int64_t T, int64_t K, bool vec, double* part, double* acc_abs,
                       double* acc_sq, hipStream_t stream) {
    const int64_t nblk = (T + kRowBlock - 1) / kRowBlock;
    const bool stats = acc_abs != nullptr;
    double* p0 = part;
    double* p1 = part ? part + nblk * K : nullptr;
    if (vec) {
        const dim3 grid((unsigned)((K + kColTile - 1) / kColTile), (unsigned)nblk);
        if (stats) hipLaunchKernelGGL((calib_tile_kernel<F, PROD, true>), grid, dim3(256), 0, stream, p, T, K, p0, p1);
        else hipLaunchKernelGGL((calib_tile_kernel<F, PROD, false>), grid, dim3(256), 0, stream, p, T, K, p0, p1);
    } else {
        const dim3 grid((unsigned)((K + 255) / 256), (unsigned)nblk);
        if (stats) hipLaunchKernelGGL((calib_col_kernel<F, PROD, true>), grid, dim3(256), 0, stream, p, T, K, p0, p1);
        else hipLaunchKernelGGL((calib_col_kernel<F, PROD, false>), grid, dim3(256), 0, stream, p, T, K, p0, p1);
    }
    if (hipError_t e = hipPeekAtLastError()) return e;
    if (!stats) return hipSuccess;
    hipLaunchKernelGGL(acc_add_kernel, dim3((unsigned)((K + 255) / 256), 2), dim3(256), 0, stream, part, nblk, K,
                       acc_abs, acc_sq);
    return hipPeekAtLastError();
}

template <typename F>
hipError_t launch_rms(const void* x, int64_t T, int64_t H, float eps, float* r, bool vec, hipStream_t stream) {
    const dim3 grid((unsigned)((T + 3) / 4));
    if (vec) hipLaunchKernelGGL((rms_rows_kernel<F, true>), grid, dim3(256), 0, stream, x, T, H, eps, r);
    else hipLaunchKernelGGL((rms_rows_kernel<F, false>), grid, dim3(256), 0, stream, x, T, H, eps, r);
    return hipPeekAtLastError();
}

#define AWQ_CALIB_FMT(dtype, CALL)                                     \
    switch (dtype) {                                                   \
    case AWQ_DTYPE_BF16: { typedef FmtBF16 F; return CALL; }           \
    case AWQ_DTYPE_F16: { typedef FmtF16 F; return CALL; }             \
    default: { typedef FmtF32 F; return CALL; }                        \
    }

hipError_t run_accum(int dtype, const ProdArgs& p, int64_t T, int64_t K, bool vec, double* part, double* a0,
                     double* a1, hipStream_t s) {
    AWQ_CALIB_FMT(dtype, (launch_prod<F, PROD_PLAIN>(p, T, K, vec, part, a0, a1, s)))
}
hipError_t run_norm(int dtype, const ProdArgs& p, int64_t T, int64_t K, bool vec, double* part, double* a0,
                    double* a1, hipStream_t s) {
    AWQ_CALIB_FMT(dtype, (launch_prod<F, PROD_NORM>(p, T, K, vec, part, a0, a1, s)))
}
hipError_t run_swiglu(int dtype, const ProdArgs& p, int64_t T, int64_t K, bool vec, double* part, double* a0,
                      double* a1, hipStream_t s) {
    AWQ_CALIB_FMT(dtype, (launch_prod<F, PROD_SWIGLU>(p, T, K, vec, part, a0, a1, s)))
}
hipError_t run_rms(int dtype, const void* x, int64_t T, int64_t H, float eps, float* r, bool vec, hipStream_t s) {
    AWQ_CALIB_FMT(dtype, (launch_rms<F>(x, T, H, eps, r, vec, s)))
}
#undef AWQ_CALIB_FMT

constexpr int64_t kMaxTokens = (int64_t)65535 * kRowBlock;   // one grid dimension of 256-token blocks

// the checks the three entries share, in the documented order; 1 = empty (AWQ_OK, nothing to do)
int check_calib(const char* what, int dtype, int64_t tokens, int64_t K, int64_t tokens_before, int* empty) {
    *empty = 0;
    if (dtype != AWQ_DTYPE_BF16 && dtype != AWQ_DTYPE_F16 && dtype != AWQ_DTYPE_F32)
        return fail(AWQ_EUNSUPPORTED, "%s takes bf16 / fp16 / fp32 activations (dtype code %d)", what, dtype);
    if (tokens < 0 || K < 0 || tokens_before < 0)
        return fail(AWQ_EINVAL, "%s: negative shape (tokens=%lld, K=%lld, tokens_before=%lld)", what,
                    (long long)tokens, (long long)K, (long long)tokens_before);
    if (tokens == 0 || K == 0) {
        *empty = 1;
        return AWQ_OK;
    }
    if (tokens_before % kRowBlock != 0)
        return fail(AWQ_EINVAL, "%s: tokens_before (%lld) must be a multiple of %d: every call on an accumulator "
                                "but the last adds whole 256-token blocks", what, (long long)tokens_before, kRowBlock);
    if (tokens > kMaxTokens || K > ((int64_t)1 << 31) || tokens > ((int64_t)1 << 60) / K)
        return fail(AWQ_EINVAL, "%s: shape too large (tokens=%lld, K=%lld)", what, (long long)tokens, (long long)K);
    return AWQ_OK;
}

}  // namespace
}  // namespace awq

using awq::aligned;
using awq::fail;

extern "C" {

int awq_act_stats_accum(const void* x, int dtype, int64_t tokens, int64_t K, int64_t row_stride,
                        int64_t tokens_before, double* work, double* acc_abs, double* acc_sq, void* stream) {
    awq::set_error(AWQ_OK, "");
    int empty;
    if (int rc = awq::check_calib("awq_act_stats_accum", dtype, tokens, K, tokens_before, &empty)) return rc;
    if (empty) return AWQ_OK;
    if (row_stride < K) return fail(AWQ_EINVAL, "awq_act_stats_accum: row_stride (%lld) smaller than K (%lld)",
                                    (long long)row_stride, (long long)K);
    if (!x || !work || !acc_abs || !acc_sq) return fail(AWQ_EINVAL, "null argument");
    const bool vec = K % 8 == 0 && row_stride % 8 == 0 && aligned(x, 16);
    awq::ProdArgs p{x, nullptr, nullptr, nullptr, row_stride, 0};
    return awq::hip_status(awq::run_accum(dtype, p, tokens, K, vec, work, acc_abs, acc_sq, (hipStream_t)stream),
                           "awq act stats accum");
}

int awq_rmsnorm_stats(const void* x, int dtype, int64_t tokens, int64_t H, const void* weight, float eps, void* out,
                      int64_t tokens_before, double* work, double* acc_abs, double* acc_sq, void* stream) {
    awq::set_error(AWQ_OK, "");
    int empty;
    if (int rc = awq::check_calib("awq_rmsnorm_stats", dtype, tokens, H, tokens_before, &empty)) return rc;
    if (empty) return AWQ_OK;
    if (H > ((int64_t)1 << 24)) return fail(AWQ_EINVAL, "awq_rmsnorm_stats: H (%lld) above 2^24", (long long)H);
    if (!x || !weight || !out || !work) return fail(AWQ_EINVAL, "null argument");
    if ((acc_abs == nullptr) != (acc_sq == nullptr))
        return fail(AWQ_EINVAL, "awq_rmsnorm_stats: acc_abs and acc_sq are given together or not at all");
    if (out == x) return fail(AWQ_EINVAL, "awq_rmsnorm_stats: out may not alias x (x is read twice)");
    float* r = (float*)work;
    double* part = work + (tokens + 1) / 2;
    const bool vec_x = H % 8 == 0 && aligned(x, 16);
    if (hipError_t e = awq::run_rms(dtype, x, tokens, H, eps, r, vec_x, (hipStream_t)stream))
        return awq::hip_status(e, "awq rmsnorm rows");
    const bool vec = vec_x && aligned(weight, 16) && aligned(out, 16);
    awq::ProdArgs p{x, weight, r, out, H, 0};
    return awq::hip_status(awq::run_norm(dtype, p, tokens, H, vec, part, acc_abs, acc_sq, (hipStream_t)stream),
                           "awq rmsnorm stats");
}

int awq_swiglu_stats(const void* gate, const void* up, int dtype, int64_t tokens, int64_t K, int64_t row_stride,
                     void* out, int64_t tokens_before, double* work, double* acc_abs, double* acc_sq, void* stream) {
    awq::set_error(AWQ_OK, "");
    int empty;
    if (int rc = awq::check_calib("awq_swiglu_stats", dtype, tokens, K, tokens_before, &empty)) return rc;
    if (empty) return AWQ_OK;
    if (row_stride < K) return fail(AWQ_EINVAL, "awq_swiglu_stats: row_stride (%lld) smaller than K (%lld)",
                                    (long long)row_stride, (long long)K);
    if (!gate || !up || !out) return fail(AWQ_EINVAL, "null argument");
    if ((acc_abs == nullptr) != (acc_sq == nullptr))
        return fail(AWQ_EINVAL, "awq_swiglu_stats: acc_abs and acc_sq are given together or not at all");
    if (acc_abs && !work) return fail(AWQ_EINVAL, "null argument");
    const bool vec = K % 8 == 0 && row_stride % 8 == 0 && aligned(gate, 16) && aligned(up, 16) && aligned(out, 16);
    awq::ProdArgs p{gate, up, nullptr, out, row_stride, row_stride};
    return awq::hip_status(awq::run_swiglu(dtype, p, tokens, K, vec, work, acc_abs, acc_sq, (hipStream_t)stream),
                           "awq swiglu stats");
}

}  // extern "C"
