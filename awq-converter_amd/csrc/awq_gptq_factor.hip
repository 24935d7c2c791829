// awq_gptq_factor.hip — the factor GPTQ's solver reads: U upper triangular with
// (H + damp mean(diag H) I)^-1 = U^T U, in place over the fp32 Hessian (include/awq_hip.h
// awq_gptq_factor).
//
// Two sweeps over the block columns of 128, 2 K^3 / 3 flops together:
//   1. H_d = R R^T with R UPPER triangular (a Cholesky run from the last column to the first),
//      blocked and right-looking, block columns j from the last to the first:
//        diag      one workgroup: the updated block (j, j) in LDS is factored bottom-up into R_jj and
//                  inverted by back-substitution; U_jj = R_jj^-1 replaces the block (R_jj itself is
//                  not needed again), its strict lower part written as zeros;
//        panel     R_ij = H_ij U_jj^T for the block rows i < j: a GEMM, since the inverse is explicit;
//                  the same launch zero-fills the tiles (i, j), i > j, below the diagonal;
//        trailing  H_ik -= R_ij R_kj^T for i <= k < j, a grid over the triangle's tiles.
//   2. U = R^-1 in place, block columns k from the first to the last.  Before step k the leading
//      k x k blocks hold R_TL^-1, the blocks right of them -R_TL^-1 R_TR, the rest R:
//        row       A_kj = -U_kk A_kj for j > k;
//        rect      A_ij += A_ik A_kj for i < k < j: a rank-128 update of a rectangle, as wide a grid
//                  as the trailing update's (a left-looking back-substitution would launch one block
//                  column at a time);
//        column    A_ik = A_ik U_kk for i < k.
// Every launch's tiles read only tiles no tile of the same launch writes, except their own (read
// whole before it is written), so the stream's order of launches is the only synchronisation.
//
// One tile kernel serves all five GEMMs: a 128 x 128 output tile with a 128-deep reduction on
// v_mfma_f32_32x32x2_f32, fp32 operands and accumulation.  4 waves, each a 64 x 64 quarter (2 x 2
// accumulators of 32 x 32).  The reduction goes through LDS in 4 slices of 32: the next slice's 16-B
// global loads are in flight while the current one is multiplied; A is staged [m][k] (row stride 36
// floats), B [n][k] for A B^T and [k][n] (stride 160) for A B.  Rows and columns past K read zeros
// and are not stored, so a last block of 32, 64 or 96 columns needs no kernel of its own.
#include "awq_lanes.h"

namespace awq {
namespace {

constexpr int kB = 128;         // the block: the rounding kernel's (awq_gptq_round.hip)
constexpr int kLd = kB + 1;     // the diagonal kernel's LDS row stride: rows and columns both conflict-free
constexpr int kKC = 32;         // reduction slice of the tile kernel
constexpr int kAS = kKC + 4;    // LDS row stride of a [128][32] slice (16-B aligned rows)
constexpr int kBS = kB + 32;    // LDS row stride of a [32][128] slice

typedef float f16v __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------
// The diagonal: dead columns, the mean and the damping.  Two launches of one workgroup of 128 lanes
// per block of 128 diagonal entries.  Sum order (fixed): a block's entries in double by the tree
// lane l += lane l + 64, + 32, ... + 1; the block sums in double, lane l taking blocks l, l + 128, ...
// in ascending order, then the same tree.  Every workgroup of the second launch repeats that sum, so
// all add the same shift.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double tree128(double v, double* sh, int tid) {
    sh[tid] = v;
#pragma unroll
    for (int s = 64; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) sh[tid] = sh[tid] + sh[tid + s];
    }
    __syncthreads();
    return sh[0];
}

__global__ __launch_bounds__(128) void factor_diag_sum_kernel(float* __restrict__ h, int64_t K,
                                                              double* __restrict__ part) {
    __shared__ double sh[kB];
    const int tid = threadIdx.x;
    const int64_t d = (int64_t)blockIdx.x * kB + tid;
    float v = 0.0f;
    if (d < K) {
        v = h[d * K + d];
        if (v == 0.0f) {                      // a dead column
            v = 1.0f;
            h[d * K + d] = v;
        }
    }
    const double s = tree128((double)v, sh, tid);
    if (tid == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(128) void factor_damp_kernel(float* __restrict__ h, int64_t K, float damp,
                                                          const double* __restrict__ part, int64_t n_blocks,
                                                          int32_t* __restrict__ status) {
    __shared__ double sh[kB];
    const int tid = threadIdx.x;
    double v = 0.0;
    for (int64_t b = tid; b < n_blocks; b += kB) v = v + part[b];
    const double mean = tree128(v, sh, tid) / (double)K;
    const float shift = (float)((double)damp * mean);
    const int64_t d = (int64_t)blockIdx.x * kB + tid;
    if (d < K) h[d * K + d] = h[d * K + d] + shift;
    if (blockIdx.x == 0 && tid == 0) *status = 0;
}

// ---------------------------------------------------------------------------------------
// The diagonal block (rows and columns [b0, b0 + nb), nb a multiple of 32): one workgroup of 256.
//   factor   for c = nb - 1 .. 0: r = sqrt(pivot); column c above the diagonal divided by r (a lane
//            per row); the rank-1 update of the triangle left of and above it on a 16 x 16 lane grid.
//            Two barriers per column; sqrt(pivot) goes to a side array, so the word all lanes read the
//            pivot from is written only by the previous column's update, before a barrier.  A pivot that is not a finite positive number is recorded and
//            replaced by 1: the loop runs on, its values mean nothing.
//   invert   X = R^-1 by back-substitution, a lane pair per column (the pair halves the sum over k
//            and meets through one cross-half swap), rows from the diagonal upwards.
// Only the block's upper triangle is read.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void factor_diag_kernel(float* __restrict__ h, int64_t K, int64_t b0, int nb,
                                                          int32_t* __restrict__ status) {
    __shared__ float R[kB * kLd];
    __shared__ float X[kB * kLd];
    __shared__ float vcol[kB];
    __shared__ float rdiag[kB];               // R's diagonal: R[c][c] itself keeps the pivot every lane reads
    const int tid = threadIdx.x;
    float* blk = h + b0 * K + b0;
    for (int idx = tid; idx < kB * (kB / 4); idx += 256) {
        const int r = idx >> 5, c4 = (idx & 31) * 4;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r < nb && c4 < nb && c4 + 3 >= r) v = *(const float4*)(blk + (int64_t)r * K + c4);
        float* o = R + r * kLd + c4;
        o[0] = c4 >= r ? v.x : 0.0f;
        o[1] = c4 + 1 >= r ? v.y : 0.0f;
        o[2] = c4 + 2 >= r ? v.z : 0.0f;
        o[3] = c4 + 3 >= r ? v.w : 0.0f;
    }
    __syncthreads();

    int bad = -1;                             // the first refused pivot's column (workgroup-uniform)
    const int ti = tid & 15, tk = tid >> 4;
    for (int c = nb - 1; c >= 0; --c) {
        float p = R[c * kLd + c];
        if (!(p > 0.0f && p < __builtin_inff())) {
            if (bad < 0) bad = c;
            p = 1.0f;
        }
        const float r = __builtin_sqrtf(p);
        if (tid < c) {
            const float v = R[tid * kLd + c] / r;
            R[tid * kLd + c] = v;
            vcol[tid] = v;
        } else if (tid == c) {
            rdiag[c] = r;                     // not into R[c][c]: other waves may still be reading the pivot
        }
        __syncthreads();
        for (int i = ti; i < c; i += 16) {
            const float vi = vcol[i];
            float* row = R + i * kLd;
            for (int k = i + ((tk - i) & 15); k < c; k += 16) row[k] = __builtin_fmaf(-vi, vcol[k], row[k]);
        }
        __syncthreads();
    }
    if (bad >= 0 && tid == 0 && *status == 0) *status = (int32_t)(1 + b0 + bad);   // the one workgroup of this step

    // X[i][c] = -(sum_{i < k <= c} R[i][k] X[k][c]) / rdiag[i], X[c][c] = 1 / rdiag[c]
    const int lane = tid & 63, half = lane >> 5, c = (tid >> 6) * 32 + (lane & 31);
    if (half == 0 && c < nb) X[c * kLd + c] = 1.0f / rdiag[c];
    __syncthreads();
    for (int i = nb - 2; i >= 0; --i) {
        float s = 0.0f;
        if (i < c && c < nb) {
            const float* row = R + i * kLd;
#pragma unroll 4
            for (int k = i + 1 + half; k <= c; k += 2) s = __builtin_fmaf(row[k], X[k * kLd + c], s);
        }
        float a, b;
        swap32(s, a, b);
        if (half == 0 && i < c && c < nb) X[i * kLd + c] = -(a + b) / rdiag[i];
        __syncthreads();
    }
    for (int idx = tid; idx < kB * (kB / 4); idx += 256) {
        const int r = idx >> 5, c4 = (idx & 31) * 4;
        if (r < nb && c4 < nb) {
            const float* x = X + r * kLd + c4;
            *(float4*)(blk + (int64_t)r * K + c4) = make_float4(c4 >= r ? x[0] : 0.0f, c4 + 1 >= r ? x[1] : 0.0f,
                                                                 c4 + 2 >= r ? x[2] : 0.0f, c4 + 3 >= r ? x[3] : 0.0f);
        }
    }
}

// ---------------------------------------------------------------------------------------
// The tile GEMM.  C = (ACC ? C : 0) + sign A op(B) on 128 x 128 tiles of h given by their top-left
// (row, column); NT: op(B) = B^T.  sign = -1 negates A's operand on its way out of LDS (exact; LDS keeps
// A as it is, since with same it is B too).  same: B is A (a diagonal tile of the trailing update),
// staged once.  K % 4 == 0 and h 16-B aligned: a 16-B
// piece is wholly inside the matrix or wholly outside.
// ---------------------------------------------------------------------------------------
struct Tile {
    int64_t r, c;
};

__device__ __forceinline__ float4 load4(const float* __restrict__ h, int64_t K, int64_t r, int64_t c) {
    if (r < K && c < K) return *(const float4*)(h + r * K + c);
    return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

template <bool NT>
__device__ __forceinline__ void load_slice(const float* __restrict__ h, int64_t K, Tile a, Tile b, bool same, int q,
                                           int tid, float4 (&ga)[4], float4 (&gb)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int idx = tid + 256 * p;
        ga[p] = load4(h, K, a.r + (idx >> 3), a.c + kKC * q + (idx & 7) * 4);
        if (NT) {
            if (!same) gb[p] = load4(h, K, b.r + (idx >> 3), b.c + kKC * q + (idx & 7) * 4);
        } else {
            gb[p] = load4(h, K, b.r + kKC * q + (idx >> 5), b.c + (idx & 31) * 4);
        }
    }
}

template <bool NT, bool ACC>
__device__ __forceinline__ void tile_gemm(float* __restrict__ h, int64_t K, Tile a, Tile b, Tile c, float sign, bool same,
                                          float* __restrict__ As, float* __restrict__ Bs) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
    float4 ga[4], gb[4];
    load_slice<NT>(h, K, a, b, same, 0, tid, ga, gb);

    // accumulator (mi, ni), register v of lane (r, hh): row wm + 32 mi + 8 (v >> 2) + 4 hh + (v & 3),
    // column wn + 32 ni + r of the tile; offsets inside a tile fit 32 bits (128 K < 2^28)
    float* ct = h + c.r * K + c.c;
    const uint32_t ldc = (uint32_t)K;
    const int rows = (int)(K - c.r < kB ? K - c.r : kB), cols = (int)(K - c.c < kB ? K - c.c : kB);
    f16v acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = wm + 32 * mi + 8 * (v >> 2) + 4 * hh + (v & 3), col = wn + 32 * ni + r;
                acc[mi][ni][v] = (ACC && row < rows && col < cols) ? ct[(uint32_t)row * ldc + (uint32_t)col] : 0.0f;
            }

    const float* bs = (NT && same) ? As : Bs;
    for (int q = 0; q < kB / kKC; ++q) {
        if (q) __syncthreads();               // the previous slice has been read
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int idx = tid + 256 * p;
            *(float4*)(As + (idx >> 3) * kAS + (idx & 7) * 4) = ga[p];
            if (NT) {
                if (!same) *(float4*)(Bs + (idx >> 3) * kAS + (idx & 7) * 4) = gb[p];
            } else {
                *(float4*)(Bs + (idx >> 5) * kBS + (idx & 31) * 4) = gb[p];
            }
        }
        __syncthreads();
        if (q + 1 < kB / kKC) load_slice<NT>(h, K, a, b, same, q + 1, tid, ga, gb);
#pragma unroll
        for (int s = 0; s < kKC / 2; ++s) {
            const int kk = 2 * s + hh;        // A: lane (r, hh) holds A[row r][k = hh]; B: B[k = hh][column r]
            const float a0 = sign * As[(wm + r) * kAS + kk], a1 = sign * As[(wm + 32 + r) * kAS + kk];
            float b0, b1;
            if (NT) {
                b0 = bs[(wn + r) * kAS + kk];
                b1 = bs[(wn + 32 + r) * kAS + kk];
            } else {
                b0 = bs[kk * kBS + wn + r];
                b1 = bs[kk * kBS + wn + 32 + r];
            }
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // every load of A and B by the workgroup was stored to LDS before the last slice's barrier: C may
    // be one of them
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = wm + 32 * mi + 8 * (v >> 2) + 4 * hh + (v & 3), col = wn + 32 * ni + r;
                if (row < rows && col < cols) ct[(uint32_t)row * ldc + (uint32_t)col] = acc[mi][ni][v];
            }
}

constexpr int kTileLds = kB * kAS + (kB * kAS > kKC * kBS ? kB * kAS : kKC * kBS);   // floats

// step j of the factorisation.  Block i of the grid: i < j the panel tile R_ij = H_ij U_jj^T, i > j
// zeros into the tile (i, j) below the diagonal.
__global__ __launch_bounds__(256) void factor_panel_kernel(float* __restrict__ h, int64_t K, int64_t j) {
    __shared__ __attribute__((aligned(16))) float lds[kTileLds];
    const int64_t i = blockIdx.x;
    if (i == j) return;
    if (i < j) {
        const Tile t = {i * kB, j * kB}, d = {j * kB, j * kB};
        tile_gemm<true, false>(h, K, t, d, t, 1.0f, false, lds, lds + kB * kAS);
        return;
    }
    for (int idx = threadIdx.x; idx < kB * (kB / 4); idx += 256) {
        const int64_t r = i * kB + (idx >> 5), c = j * kB + (idx & 31) * 4;
        if (r < K && c < K) *(float4*)(h + r * K + c) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// tile t of the triangle i <= k < n, counted along k: t = k (k + 1) / 2 + i
__device__ __forceinline__ void triangle_tile(int64_t t, int64_t& i, int64_t& k) {
    k = (int64_t)((__builtin_sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (k * (k + 1) / 2 > t) --k;
    while ((k + 1) * (k + 2) / 2 <= t) ++k;
    i = t - k * (k + 1) / 2;
}

// H_ik -= R_ij R_kj^T, i <= k < j
__global__ __launch_bounds__(256) void factor_trailing_kernel(float* __restrict__ h, int64_t K, int64_t j) {
    __shared__ __attribute__((aligned(16))) float lds[kTileLds];
    int64_t i, k;
    triangle_tile(blockIdx.x, i, k);
    const Tile a = {i * kB, j * kB}, b = {k * kB, j * kB}, c = {i * kB, k * kB};
    tile_gemm<true, true>(h, K, a, b, c, -1.0f, i == k, lds, lds + kB * kAS);
}

// step k of the inversion.  WHICH 0: A_kj = -U_kk A_kj, block x -> j = k + 1 + x;  1: A_ij += A_ik A_kj,
// block (x, y) -> j = k + 1 + x, i = y;  2: A_ik = A_ik U_kk, block x -> i = x.
template <int WHICH>
__global__ __launch_bounds__(256) void factor_invert_kernel(float* __restrict__ h, int64_t K, int64_t k) {
    __shared__ __attribute__((aligned(16))) float lds[kTileLds];
    const Tile d = {k * kB, k * kB};
    if (WHICH == 0) {
        const Tile t = {k * kB, (k + 1 + blockIdx.x) * kB};
        tile_gemm<false, false>(h, K, d, t, t, -1.0f, false, lds, lds + kB * kAS);
    } else if (WHICH == 1) {
        const int64_t i = blockIdx.y, j = k + 1 + blockIdx.x;
        const Tile a = {i * kB, k * kB}, b = {k * kB, j * kB}, c = {i * kB, j * kB};
        tile_gemm<false, true>(h, K, a, b, c, 1.0f, false, lds, lds + kB * kAS);
    } else {
        const Tile t = {(int64_t)blockIdx.x * kB, k * kB};
        tile_gemm<false, false>(h, K, t, d, t, 1.0f, false, lds, lds + kB * kAS);
    }
}

}  // namespace
}  // namespace awq

extern "C" int64_t awq_gptq_factor_workspace(int64_t K) {
    return K <= 0 ? 0 : (K + awq::kB - 1) / awq::kB * (int64_t)sizeof(double);
}

extern "C" int awq_gptq_factor(float* h, int64_t K, float damp, float* workspace, int64_t workspace_bytes,
                               int32_t* status, void* stream) {
    using namespace awq;
    set_error(AWQ_OK, "");
    if (K < 0) return fail(AWQ_EINVAL, "negative size (K=%lld)", (long long)K);
    if (!(damp > 0.0f && damp < 1.0f)) return fail(AWQ_EINVAL, "damp must be a finite number in (0, 1): %g", (double)damp);
    if (K == 0) return AWQ_OK;
    if (K > (int64_t)0x7FFFFFFF || K >= ((int64_t)1 << 21))
        return fail(AWQ_EUNSUPPORTED, "awq_gptq_factor: K is limited to 2^31 - 1 and K^2 to below 2^42 (K=%lld)",
                    (long long)K);
    if (K % 32 != 0) return fail(AWQ_EUNSUPPORTED, "awq_gptq_factor takes K a multiple of 32: %lld", (long long)K);
    if (!h || !workspace || !status) return fail(AWQ_EINVAL, "null argument: h, workspace and status are all needed");
    if (!aligned(h, 16) || !aligned(workspace, 8) || !aligned(status, 4))
        return fail(AWQ_EINVAL, "awq_gptq_factor: h must be 16-B aligned, workspace 8-B, status 4-B");
    if (workspace_bytes < awq_gptq_factor_workspace(K))
        return fail(AWQ_EINVAL, "awq_gptq_factor: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)awq_gptq_factor_workspace(K));
    hipStream_t st = (hipStream_t)stream;
    const int64_t nblk = (K + kB - 1) / kB;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(factor_diag_sum_kernel, dim3((unsigned)nblk), dim3(128), 0, st, h, K, part);
    hipLaunchKernelGGL(factor_damp_kernel, dim3((unsigned)nblk), dim3(128), 0, st, h, K, damp, part, nblk, status);
    for (int64_t j = nblk - 1; j >= 0; --j) {
        const int nb = (int)std::min<int64_t>(kB, K - j * kB);
        hipLaunchKernelGGL(factor_diag_kernel, dim3(1), dim3(256), 0, st, h, K, j * kB, nb, status);
        if (nblk > 1) hipLaunchKernelGGL(factor_panel_kernel, dim3((unsigned)nblk), dim3(256), 0, st, h, K, j);
        if (j > 0)
            hipLaunchKernelGGL(factor_trailing_kernel, dim3((unsigned)(j * (j + 1) / 2)), dim3(256), 0, st, h, K, j);
    }
    for (int64_t k = 0; k < nblk; ++k) {
        const unsigned right = (unsigned)(nblk - 1 - k), above = (unsigned)k;
        if (right) hipLaunchKernelGGL(factor_invert_kernel<0>, dim3(right), dim3(256), 0, st, h, K, k);
        if (right && above) hipLaunchKernelGGL(factor_invert_kernel<1>, dim3(right, above), dim3(256), 0, st, h, K, k);
        if (above) hipLaunchKernelGGL(factor_invert_kernel<2>, dim3(above), dim3(256), 0, st, h, K, k);
    }
    return hip_status(hipPeekAtLastError(), "awq gptq factor kernels");
}
