// awq_outerr.hip — output-space error on token samples (awq_output_error, include/awq_hip.h):
// E = (W^ - W) X^T and R = W X^T for a packed result W^ against the original weights W [N, K] and
// samples X [T, K], reduced to err_sq[n] = sum_t E^2 and ref_sq[n] = sum_t R^2.  The project's
// GEMM-shaped (MFMA) code.  Self-contained: the two entry points, their validation and kernels.
//
// Per element (the definition every implementation restates):
//   dq = fp32(fp16(fp16(q - z) * s))   (§5.7's reference dequantize: awq_qerror.hip)
//   w^ = dq, or RN_f32(dq / col_scale[k]) (IEEE division);  d = RN_f32(w^ - fp32(w)), no contraction
//   E[n, t] = sum_k d[n, k] x[t, k],  R[n, t] = sum_k w[n, k] x[t, k]: fp32 accumulation in the
//   matrix core's own order — the contract is a bound (include/awq_hip.h), not bits.
// Both operands are k-contiguous (W [N, K], X [T, K]): a lane's fragment is 8 (bf16) or 1 (f32)
// consecutive k of one row, the A and B lane maps as they are — an "NT" product, no transpose.
// The sums over t: every (T-tile of 128 tokens, row) gives one fp32 partial into `work` — the
// tile's tokens in a fixed in-register order, then the xor butterfly over the lanes that hold one
// row — and outerr_sum_kernel adds the T-tiles in ascending order: no atomics, the same bits
// from run to run.
#include <algorithm>

#include "awq_quant.h"

namespace awq {
namespace {

typedef __bf16 bf8v __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kTokTile = 128;    // tokens per T-tile (both kernels: one partial per T-tile and row)
constexpr int kRowTile = 128;    // fast kernel: rows per workgroup (4 waves x 32)
constexpr int kSlice = 32;       // fast kernel: k per staged slice (two 32x32x16 k-steps)
constexpr int kXRow = (kSlice + 8) * 2;            // bytes of a staged token row: 64 + 16 of padding
constexpr int kXBytes = kTokTile * kXRow;          // the X slice
constexpr int kBufBytes = kXBytes + kSlice * 4;    // + the slice's col_scale (fp32)
constexpr int kGenRows = 64;     // generic kernel: rows per workgroup (4 waves x 16)
constexpr int64_t kMaxDesc = (int64_t)1 << 22;     // fast kernel: K and x_row_stride below this keep
                                                   // a tile's buffer ranges and offsets below 2^31

// Fields 2t, 2t+1 of a chunk's qweight word(s) as the fp16 pair (1024 + f0, 1024 + f1): the
// restatement of awq_qerror.hip's field_pair (that file keeps its own: its assembly text is pinned)
template <int BITS, int QW>
__device__ __forceinline__ h2v qfield_pair(const uint32_t (&qw)[QW], int t) {
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

// ---------------------------------------------------------------------------------------
// Fast kernel: bf16, group_size in {32, 64, 128, 256}, 16-B aligned w / x / qweight,
// x_row_stride % 8 == 0.  v_mfma_f32_32x32x16_bf16.  A workgroup of 4 waves takes a 128-row x
// 128-token tile; wave v owns rows 32 v .. 32 v + 31 and all 128 tokens (4 accumulators of 32 x
// 32, and 4 more for R).  Lane l (r = l & 31, h = l >> 5) holds A[row r][k = 8 h + j]: its 16 B
// of w, the matching qweight word(s) and the group's scale / zero point give d for those 8 k in
// registers (packed-fp16 dq, the optional division, the subtraction), split into d_hi = RN_bf16(d),
// d_lo = RN_bf16(d - d_hi): two MFMAs per k-step into one accumulator (bf16 x bf16 products are
// exact in fp32), a third (w x) into the second when ref_sq is asked for.  The X slice [128
// tokens][32 k] and the slice's col_scale go through LDS (two buffers, one barrier per slice);
// B[k = 8 h + j][col r] is one 16-B read of token row r.  Rows and tokens past the end read
// zeros (buffer descriptors sized to the tile's rows; predicates for scales / qzeros) and their
// stores are dropped.
// ---------------------------------------------------------------------------------------
struct ARaw {
    u4 w[2];              // the lane's 8 weights of k-steps 0 and 1
    uint32_t qw[2][2];    // their qweight words
    uint32_t sbits, zw;   // the slice's group: fp16 scale bits, qzeros word
};

template <int BITS>
__device__ __forceinline__ ARaw load_a(const __amdgpu_buffer_rsrc_t rw, const __amdgpu_buffer_rsrc_t rq,
                                       const uint16_t* __restrict__ scales, const uint32_t* __restrict__ qzeros,
                                       uint32_t row, bool row_ok, int64_t grow, uint32_t K, int64_t G, int64_t zpr,
                                       uint32_t k0, int h, int gs_shift) {
    constexpr int PER = 32 / BITS;
    ARaw a;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint32_t k = k0 + 16u * s + 8u * h;
        a.w[s] = __builtin_amdgcn_raw_buffer_load_b128(rw, (row * K + k) * 2u, 0, 0);
        const uint32_t qoff = (row * (K / PER) + k / PER) * 4u;
        if constexpr (BITS == 4) {
            a.qw[s][0] = __builtin_amdgcn_raw_buffer_load_b32(rq, qoff, 0, 0);
            a.qw[s][1] = 0;
        } else {
            const u2v t = __builtin_amdgcn_raw_buffer_load_b64(rq, qoff, 0, 0);
            a.qw[s][0] = t.x;
            a.qw[s][1] = t.y;
        }
    }
    const int64_t g = k0 >> gs_shift;
    a.sbits = row_ok ? scales[grow * G + g] : 0u;
    a.zw = row_ok ? qzeros[grow * zpr + g / PER] : 0u;
    return a;
}

template <int BITS, bool DIV, bool REF>
__global__ __launch_bounds__(256) void outerr_mfma_kernel(const void* __restrict__ w,
                                                          const uint32_t* __restrict__ qweight,
                                                          const uint32_t* __restrict__ qzeros,
                                                          const uint16_t* __restrict__ scales,
                                                          const float* __restrict__ col_scale,
                                                          const void* __restrict__ x, int64_t N, int64_t K, int64_t T,
                                                          int64_t xs, int gs_shift, int64_t t_tiles, int64_t tiles,
                                                          float* __restrict__ work, float* __restrict__ err) {
    constexpr int PER = 32 / BITS, QW = BITS / 4;
    constexpr uint32_t MASK = (1u << BITS) - 1u;
    __shared__ __attribute__((aligned(16))) char lds[2 * kBufBytes];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
    const int64_t G = K >> gs_shift, zpr = (G + PER - 1) / PER, wpr = K / PER;
    const uint32_t Ku = (uint32_t)K, xsu = (uint32_t)xs, nk = Ku / kSlice;
    const uint32_t row = 32u * wv + r;

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t nt = tile / t_tiles, tt = tile - nt * t_tiles;
        const int64_t n0 = nt * kRowTile, t0 = tt * kTokTile;
        const uint32_t nn = (uint32_t)min((int64_t)kRowTile, N - n0), tn = (uint32_t)min((int64_t)kTokTile, T - t0);
        const __amdgpu_buffer_rsrc_t rw = rsrc((const char*)w + n0 * K * 2, nn * Ku * 2u);
        const __amdgpu_buffer_rsrc_t rq = rsrc(qweight + n0 * wpr, nn * (uint32_t)wpr * 4u);
        const __amdgpu_buffer_rsrc_t rx = rsrc((const char*)x + t0 * xs * 2, ((tn - 1u) * xsu + Ku) * 2u);
        const bool row_ok = row < nn;
        const int64_t grow = n0 + row;

        f16v acc[4], racc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc[j][i] = 0.0f; racc[j][i] = 0.0f; }

        // the staged part of slice k0: this thread's two 16-B pieces of X (piece c: token c >> 2,
        // k 8 (c & 3)) and, in the first 32 threads, one col_scale value
        u4 xr[2];
        float cr = 1.0f;
#define AWQ_OE_LOAD_X(k0)                                                                                   \
    {                                                                                                       \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                     \
            const uint32_t c = (uint32_t)tid + 256u * i;                                                    \
            xr[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, ((c >> 2) * xsu + (k0) + 8u * (c & 3u)) * 2u, 0, 0); \
        }                                                                                                   \
        if (DIV && tid < kSlice) cr = col_scale[(k0) + tid];                                                \
    }
#define AWQ_OE_STORE_X(buf)                                                                                 \
    {                                                                                                       \
        char* b = lds + (buf) * kBufBytes;                                                                  \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                     \
            const uint32_t c = (uint32_t)tid + 256u * i;                                                    \
            *(u4*)(b + (c >> 2) * kXRow + (c & 3u) * 16u) = xr[i];                                          \
        }                                                                                                   \
        if (DIV && tid < kSlice) *(float*)(b + kXBytes + tid * 4) = cr;                                     \
    }
        AWQ_OE_LOAD_X(0u)
        ARaw a = load_a<BITS>(rw, rq, scales, qzeros, row, row_ok, grow, Ku, G, zpr, 0u, h, gs_shift);
        AWQ_OE_STORE_X(0)
        __syncthreads();

        for (uint32_t ks = 0; ks < nk; ++ks) {
            const int cur = (int)(ks & 1u);
            const bool more = ks + 1u < nk;
            ARaw an = a;
            if (more) {
                AWQ_OE_LOAD_X((ks + 1u) * kSlice)
                an = load_a<BITS>(rw, rq, scales, qzeros, row, row_ok, grow, Ku, G, zpr, (ks + 1u) * kSlice, h, gs_shift);
            }
            const char* b = lds + cur * kBufBytes;
            // d of this lane's 8 k of each k-step, split hi / lo
            const uint32_t g = (ks * kSlice) >> gs_shift;
            const uint32_t zf = (a.zw >> (BITS * (g % PER))) & MASK;
            const h2v s2 = __builtin_bit_cast(h2v, a.sbits | (a.sbits << 16));
            const h2v zq = __builtin_bit_cast(h2v, (0x6400u + zf) * 0x10001u);
            u4 fhi[2], flo[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                Chunk<1> v;
                v.w[0] = a.w[s];
                float cs[8] = {};
                if (DIV) {
                    const f4v c0 = *(const f4v*)(b + kXBytes + (16 * s + 8 * h) * 4);
                    const f4v c1 = *(const f4v*)(b + kXBytes + (16 * s + 8 * h + 4) * 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) { cs[i] = c0[i]; cs[4 + i] = c1[i]; }
                }
                uint32_t qw[QW];
#pragma unroll
                for (int i = 0; i < QW; ++i) qw[i] = a.qw[s][i];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const h2v dq = (qfield_pair<BITS, QW>(qw, t) - zq) * s2;   // fp16(fp16(q - z) * s), two elements
                    float d0 = (float)dq.x, d1 = (float)dq.y;
                    if (DIV) { d0 = d0 / cs[2 * t]; d1 = d1 / cs[2 * t + 1]; }
                    d0 = d0 - FmtBF16::elem(v, 2 * t);
                    d1 = d1 - FmtBF16::elem(v, 2 * t + 1);
                    const uint32_t hb = __builtin_bit_cast(uint32_t, __builtin_convertvector((f2){d0, d1}, b2));
                    const float l0 = d0 - __uint_as_float(hb << 16), l1 = d1 - __uint_as_float(hb & 0xFFFF0000u);
                    fhi[s][t] = hb;
                    flo[s][t] = __builtin_bit_cast(uint32_t, __builtin_convertvector((f2){l0, l1}, b2));
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf8v ahi = __builtin_bit_cast(bf8v, fhi[s]), alo = __builtin_bit_cast(bf8v, flo[s]);
                const bf8v aw = __builtin_bit_cast(bf8v, a.w[s]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bf8v xb = __builtin_bit_cast(bf8v, *(const u4*)(b + (32 * j + r) * kXRow + (16 * s + 8 * h) * 2));
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, xb, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, xb, acc[j], 0, 0, 0);
                    if (REF) racc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aw, xb, racc[j], 0, 0, 0);
                }
            }
            if (more) AWQ_OE_STORE_X(cur ^ 1)
            __syncthreads();
            a = an;
        }
#undef AWQ_OE_LOAD_X
#undef AWQ_OE_STORE_X

        // epilogue.  Accumulator j, register i of lane (r, h): token t0 + 32 j + r, row
        // 32 wv + (i & 3) + 8 (i >> 2) + 4 h.  Sum over the tile's tokens: the four j in order, then
        // the butterfly over the 32 lanes of the half; lane r < 16 of each half stores register r's row.
        float oe = 0.0f, orf = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t rr = 32u * wv + (uint32_t)((i & 3) + 8 * (i >> 2) + 4 * h);
            float se = 0.0f, sr = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t tc = 32u * j + r;
                const float e = acc[j][i], f = racc[j][i];
                const bool in = tc < tn;
                if (err && in && rr < nn) err[(n0 + rr) * T + t0 + tc] = e;
                se = se + (in ? e * e : 0.0f);
                if (REF) sr = sr + (in ? f * f : 0.0f);
            }
            se = grp_sum<32>(se);
            if (REF) sr = grp_sum<32>(sr);
            if (r == i) { oe = se; orf = sr; }
        }
        const uint32_t orow = 32u * wv + (uint32_t)((r & 3) + 8 * (r >> 2) + 4 * h);
        if (r < 16 && orow < nn) {
            work[tt * N + n0 + orow] = oe;
            if (REF) work[(t_tiles + tt) * N + n0 + orow] = orf;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Generic kernel: every other shape the entry accepts (fp16 / fp32, group_size 8 / 16 / 512,
// element-aligned pointers, odd strides).  v_mfma_f32_16x16x4_f32 on f32 operands: d, w and x are
// converted to f32 on the way in.  A workgroup of 4 waves takes 64 rows x 128 tokens; wave v owns
// rows 16 v .. 16 v + 15 (8 accumulators of 16 x 16, 8 more for R).  Lane l holds A[row l & 15]
// [k = l >> 4] and B[k = l >> 4][col l & 15], each one element loaded (and, for A, dequantized)
// under its own bounds test.  Correct, not fast: the second implementation the tests compare the
// fast kernel with.
// ---------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ float elem_f32(const void* p, int64_t i) {
    if (DT == AWQ_DTYPE_BF16) return __uint_as_float((uint32_t)((const uint16_t*)p)[i] << 16);
    if (DT == AWQ_DTYPE_F16) return (float)((const _Float16*)p)[i];
    return ((const float*)p)[i];
}

template <int DT>
__global__ __launch_bounds__(256) void outerr_generic_kernel(const void* __restrict__ w,
                                                             const uint32_t* __restrict__ qweight,
                                                             const uint32_t* __restrict__ qzeros,
                                                             const uint16_t* __restrict__ scales,
                                                             const float* __restrict__ col_scale,
                                                             const void* __restrict__ x, int64_t N, int64_t K,
                                                             int64_t T, int64_t xs, int64_t gs, int bits,
                                                             int64_t t_tiles, int64_t tiles, int want_ref,
                                                             float* __restrict__ work, float* __restrict__ err) {
    const int per = 32 / bits;
    const uint32_t mask = (1u << bits) - 1u;
    const int64_t G = K / gs, wpr = (K + per - 1) / per, zpr = (G + per - 1) / per;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t nt = tile / t_tiles, tt = tile - nt * t_tiles;
        const int64_t n0 = nt * kGenRows + 16 * wv, t0 = tt * kTokTile;
        const int64_t n = n0 + c;
        f4v acc[8], racc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) { acc[j][i] = 0.0f; racc[j][i] = 0.0f; }
        for (int64_t k0 = 0; k0 < K; k0 += 4) {
            const int64_t k = k0 + q;       // K % 8 == 0: k < K
            float d = 0.0f, wf = 0.0f;
            if (n < N) {
                const int64_t g = k / gs;
                const float s = (float)__builtin_bit_cast(_Float16, scales[n * G + g]);
                const int z = (int)((qzeros[n * zpr + g / per] >> (bits * (int)(g % per))) & mask);
                const int f = (int)((qweight[n * wpr + k / per] >> (bits * (int)(k % per))) & mask);
                wf = elem_f32<DT>(w, n * K + k);
                float dq = (float)(_Float16)((float)(f - z) * s);   // exact product, one RNE to fp16
                if (col_scale) dq = dq / col_scale[k];
                d = dq - wf;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int64_t t = t0 + 16 * j + c;
                const float xv = t < T ? elem_f32<DT>(x, t * xs + k) : 0.0f;
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(d, xv, acc[j], 0, 0, 0);
                if (want_ref) racc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf, xv, racc[j], 0, 0, 0);
            }
        }
        // accumulator j, register i of lane (c, q): token t0 + 16 j + c, row n0 + 4 q + i
        float oe = 0.0f, orf = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t rr = n0 + 4 * q + i;
            float se = 0.0f, sr = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int64_t t = t0 + 16 * j + c;
                const float e = acc[j][i], f = racc[j][i];
                const bool in = t < T;
                if (err && in && rr < N) err[rr * T + t] = e;
                se = se + (in ? e * e : 0.0f);
                sr = sr + (in ? f * f : 0.0f);
            }
            se = grp_sum<16>(se);
            sr = grp_sum<16>(sr);
            if (c == i) { oe = se; orf = sr; }
        }
        const int64_t orow = n0 + 4 * q + c;
        if (c < 4 && orow < N) {
            work[tt * N + orow] = oe;
            if (want_ref) work[(t_tiles + tt) * N + orow] = orf;
        }
    }
}

// the T-tiles' partials of every row, added in ascending order
__global__ __launch_bounds__(256) void outerr_sum_kernel(const float* __restrict__ work, int64_t N, int64_t t_tiles,
                                                         float* __restrict__ err_sq, float* __restrict__ ref_sq) {
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) {
        float e = 0.0f, f = 0.0f;
        for (int64_t tt = 0; tt < t_tiles; ++tt) {
            e = e + work[tt * N + n];
            if (ref_sq) f = f + work[(t_tiles + tt) * N + n];
        }
        err_sq[n] = e;
        if (ref_sq) ref_sq[n] = f;
    }
}

constexpr int64_t kMaxProduct = (int64_t)1 << 60;
int64_t tok_tiles(int64_t T) { return (T + kTokTile - 1) / kTokTile; }

}  // namespace
}  // namespace awq

using namespace awq;

extern "C" int64_t awq_output_error_work_bytes(int64_t N, int64_t T) {
    if (N <= 0 || T <= 0 || N > kMaxProduct / T) return 0;
    return 2 * tok_tiles(T) * N * (int64_t)sizeof(float);   // [2 (E, R)][T-tiles][N]
}

extern "C" int awq_output_error(const void* w, int dtype, int64_t N, int64_t K, int64_t group_size, int bits,
                                int symmetric, const int32_t* qweight, const int32_t* qzeros, const uint16_t* scales,
                                const float* col_scale, const void* x, int64_t T, int64_t x_row_stride, void* work,
                                float* err_sq, float* ref_sq, float* err, void* stream) {
    (void)symmetric;   // q - z = field(qweight) - field(qzeros): qmin cancels
    set_error(AWQ_OK, "");
    if (bits != 4 && bits != 8) return fail(AWQ_EINVAL, "Unsupported bit width: %d. Supported: 4, 8.", bits);
    if (group_size <= 0) return fail(AWQ_EINVAL, "Group size must be a positive integer: %lld", (long long)group_size);
    if (N < 0 || K < 0 || T < 0)
        return fail(AWQ_EINVAL, "negative shape (%lld, %lld, %lld)", (long long)N, (long long)K, (long long)T);
    if (group_size < 8 || group_size > 512 || (group_size & (group_size - 1)))
        return fail(AWQ_EUNSUPPORTED, "awq_output_error: group_size %lld is not a power of two in [8, 512]",
                    (long long)group_size);
    if (K % group_size)
        return fail(AWQ_EUNSUPPORTED, "awq_output_error: K %lld is not a multiple of group_size %lld", (long long)K,
                    (long long)group_size);
    if (dtype == AWQ_DTYPE_F64) return fail(AWQ_EUNSUPPORTED, "awq_output_error: fp64 weights are not supported");
    if (dtype != AWQ_DTYPE_BF16 && dtype != AWQ_DTYPE_F16 && dtype != AWQ_DTYPE_F32)
        return fail(AWQ_EINVAL, "awq_output_error: dtype code %d is not a weight dtype (bf16, fp16, fp32)", dtype);
    if (x_row_stride < K)
        return fail(AWQ_EINVAL, "awq_output_error: x_row_stride %lld < K %lld", (long long)x_row_stride, (long long)K);
    if (N > 0 && (K > kMaxProduct / N || T > kMaxProduct / N || (T > 0 && x_row_stride > kMaxProduct / T)))
        return fail(AWQ_EUNSUPPORTED, "awq_output_error: %lld x %lld weights on %lld tokens exceed 2^60 elements",
                    (long long)N, (long long)K, (long long)T);
    if (N == 0 || K == 0 || T == 0) return AWQ_OK;   // empty: nothing is read or written, the pointers are not looked at
    if (!w || !qweight || !qzeros || !scales || !x || !work || !err_sq)
        return fail(AWQ_EINVAL, "awq_output_error: null argument");
    const size_t esz = dtype == AWQ_DTYPE_F32 ? 4 : 2;
    if (!aligned(w, esz) || !aligned(x, esz) || !aligned(qweight, 4) || !aligned(qzeros, 4) || !aligned(scales, 2) ||
        !aligned(col_scale, 4) || !aligned(work, 4) || !aligned(err_sq, 4) || !aligned(ref_sq, 4) || !aligned(err, 4))
        return fail(AWQ_EINVAL, "awq_output_error: a pointer is not aligned to its element size");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t* qwp = (const uint32_t*)qweight;
    const uint32_t* qzp = (const uint32_t*)qzeros;
    float* wk = (float*)work;
    const int64_t tts = tok_tiles(T);
    const bool fast = dtype == AWQ_DTYPE_BF16 && fast_group_size(group_size) && aligned(w, 16) && aligned(x, 16) &&
                      aligned(qweight, 16) && x_row_stride % 8 == 0 && K < kMaxDesc && x_row_stride < kMaxDesc;
    if (fast) {
        const int64_t tiles = (N + kRowTile - 1) / kRowTile * tts;
        const unsigned grid = diag_cap((unsigned)std::min<int64_t>(tiles, 0x7FFFFFFF));
        const int shift = __builtin_ctzll((unsigned long long)group_size);
#define AWQ_OE(BITS, DIV, REF)                                                                                     \
    hipLaunchKernelGGL((outerr_mfma_kernel<BITS, DIV, REF>), dim3(grid), dim3(256), 0, st, w, qwp, qzp, scales,      \
                       col_scale, x, N, K, T, x_row_stride, shift, tts, tiles, wk, err)
#define AWQ_OE_BITS(DIV, REF) \
    if (bits == 4) AWQ_OE(4, DIV, REF); else AWQ_OE(8, DIV, REF)
        if (col_scale) {
            if (ref_sq) { AWQ_OE_BITS(true, true); } else { AWQ_OE_BITS(true, false); }
        } else {
            if (ref_sq) { AWQ_OE_BITS(false, true); } else { AWQ_OE_BITS(false, false); }
        }
#undef AWQ_OE_BITS
#undef AWQ_OE
    } else {
        const int64_t tiles = (N + kGenRows - 1) / kGenRows * tts;
        const unsigned grid = diag_cap((unsigned)std::min<int64_t>(tiles, 0x7FFFFFFF));
#define AWQ_OE_GEN(DT)                                                                                          \
    hipLaunchKernelGGL((outerr_generic_kernel<DT>), dim3(grid), dim3(256), 0, st, w, qwp, qzp, scales, col_scale, x, \
                       N, K, T, x_row_stride, group_size, bits, tts, tiles, ref_sq ? 1 : 0, wk, err)
        if (dtype == AWQ_DTYPE_BF16) AWQ_OE_GEN(AWQ_DTYPE_BF16);
        else if (dtype == AWQ_DTYPE_F16) AWQ_OE_GEN(AWQ_DTYPE_F16);
        else AWQ_OE_GEN(AWQ_DTYPE_F32);
#undef AWQ_OE_GEN
    }
    hipError_t e = hipPeekAtLastError();
    if (e == hipSuccess) {
        const unsigned grid = (unsigned)std::min<int64_t>((N + 255) / 256, 65536);
        hipLaunchKernelGGL(outerr_sum_kernel, dim3(grid), dim3(256), 0, st, wk, N, tts, err_sq, ref_sq);
        e = hipPeekAtLastError();
    }
    return hip_status(e, "awq output error kernels");
}
