// awq_act_mxfp4.hip — the activation-aware scale search on the MXFP4 grid (include/awq_hip.h
// awq_act_search_losses_mxfp4, awq_quantize_mxfp4_scaled).  Self-contained: the two
// entry points, their validation and kernels.  The block arithmetic (scale rule, the one-addition
// E2M1 rounding) is awq_mxfp4.h's, the bits of awq_quantize_mxfp4.
//
// The loss kernel.  A workgroup of 4 waves owns a slab of 256 columns (8 blocks) and walks the rows
// in trips of 16.  The slab's slice of the scale table and of the reciprocal table is staged in LDS
// once ([candidate][scale row | reciprocal row][256], up to 32 candidates = 64 KiB; a longer grid
// runs in chunks of 32 candidates, the weights read once per chunk) and serves every row the
// workgroup visits.  A lane holds 8 consecutive elements of two rows (one 16-B load each, two for
// fp32: half a wave reads 512 contiguous bytes of a row) and the 8 x_sq values of its columns for
// the whole kernel; a block is a quad of lanes, so amax, the "mse" sums and the loss are two DPP
// quad steps each, in awq_lanes.h's order.  Candidates are the inner loop: per candidate a lane
// reads its 8 scales and 8 reciprocals from LDS (four ds_read_b128, shared by its two rows) and
// everything else is register arithmetic.
//
// Per element and candidate (every line one fp32 operation, no contraction):
//   w' = RN_D(w s); t = |w'| 2^-X, v = min(t, 6), r = v + 2^(22 + k), m = r - 2^(22 + k)  (awq_mxfp4.h)
//   dq = +-m 2^X; q = RN(dq / s); d = q - w; c = x_sq (d d); the lane's 8 c summed in order from +0,
//   then the quad's tree: (p0 + p1) + (p2 + p3).
// The loss kernel needs the rounded magnitudes only, never the codes.  q is the Markstein quotient
// (awq_quant.h mquot) where a reciprocal table is given and the block's scale byte is in [87, 167]:
// dq has a two-bit significand, a subset of the fp16 significands awq_selftest 1 proves the identity
// for, the table's in-range entries are in [2^-60, 2^60], and with |X| <= 40 no intermediate leaves
// the normal range, so the identity's scale invariance holds.  An out-of-range entry is a NaN
// reciprocal: a lane whose 8-element sum comes out NaN, or whose block is outside the byte range,
// takes the IEEE division (the same bits in range).  A block with a NaN or an inf has dq = NaN: its
// loss is NaN.
//
// The scaled quantize: awq_mxfp4.hip's quantize kernel (one wave per 2048-element segment) with
// w' = RN_D(w s[k]) formed in registers between the load and the block arithmetic; k is the flat
// index modulo K, one 64-bit remainder per segment (wave-uniform) and one conditional subtraction
// (K >= 2048) or one 32-bit remainder (K < 2048) per lane and load.
#include <algorithm>

#include "awq_mxfp4.h"

namespace awq {
namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kSlabCols = 256;    // columns of a loss workgroup: 32 lanes x 8
constexpr int kTripRows = 16;     // rows of a workgroup's trip: 4 waves x 2 loads x 2 half-waves
constexpr int kCandChunk = 32;    // candidates staged in LDS at once (64 KiB with reciprocals)
constexpr unsigned kLossGroups = 2048;   // the loss grid's target: workgroups (8 per CU)

// RN_D(w s) of two elements, as fp32 (the bits of awq_apply_input_scale): the fp32 product, then the
// format's rounding — bf16 both at once (v_cvt_pk_bf16_f32), fp16 behind a value barrier so that the
// product is rounded to fp32 first (a fused v_fma_mixlo_f16 would round once).
template <typename F>
__device__ __forceinline__ f2 scale_pair(f2 w, f2 s) {
    const f2 p = w * s;
    if constexpr (std::is_same<F, FmtBF16>::value) {
        const uint32_t h = __builtin_bit_cast(uint32_t, __builtin_convertvector(p, b2));
        return (f2){__uint_as_float(h << 16), __uint_as_float(h & 0xFFFF0000u)};
    } else if constexpr (std::is_same<F, FmtF16>::value) {
        const h2v h = __builtin_convertvector((f2){opaque(p.x), opaque(p.y)}, h2v);
        return (f2){(float)h.x, (float)h.y};
    } else {
        return p;
    }
}

// a chunk's 8 elements as fp32 pairs
template <typename F>
__device__ __forceinline__ void chunk_pairs(const Chunk<F::NW>& c, f2 (&w)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (f2){F::elem(c, 2 * i), F::elem(c, 2 * i + 1)};
}

// The rounded magnitudes of a lane's 8 elements at the scale 2^-X = inv and, with ERR, the sum of
// (t - m)^2 in element order from +0: awq_mxfp4.h's quant8 without the codes, the same operations.
template <bool ERR>
__device__ __forceinline__ void round8(const f2 (&x)[4], float inv, f2 (&m)[4], float& err) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f2 t = __builtin_elementwise_abs(x[i]) * (f2){inv, inv};
        const f2 v = __builtin_elementwise_min(t, (f2){6.0f, 6.0f});
        const uint32_t k0 = max(__float_as_uint(v.x) >> 23, 127u), k1 = max(__float_as_uint(v.y) >> 23, 127u);
        const f2 magic = {__uint_as_float((k0 + 22u) << 23), __uint_as_float((k1 + 22u) << 23)};
        const f2 r = v + magic;                                        // the one rounding
        m[i] = r - magic;
        if (ERR) {
            const f2 d = t - m[i];
            const f2 dd = d * d;
            s = s + dd.x;
            s = s + dd.y;
        }
    }
    err = s;
}

// One lane's share of a block's loss under candidate scales s (reciprocals rs): the sum over its 8
// elements, to be added over the quad by the caller.  bad: the block's loss is NaN whatever this
// returns.
template <typename F, int RULE, bool RT>
__device__ __forceinline__ float lane_loss(const f2 (&w)[4], const f2 (&s)[4], const f2 (&rs)[4], const f2 (&xs)[4],
                                           bool& bad) {
    f2 wp[4];
    uint32_t am = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        wp[i] = scale_pair<F>(w[i], s[i]);
        am = max(am, max(__float_as_uint(wp[i].x) & 0x7FFFFFFFu, __float_as_uint(wp[i].y) & 0x7FFFFFFFu));
    }
    // the block's scale byte: awq_mxfp4.h mxfp4_block on the fp32 values of w' (the exponent of a
    // D value is the exponent of its fp32 value)
    const uint32_t amax = grp_max<4, uint32_t>(am);
    bad = amax >= 0x7F800000u;
    uint32_t e = amax == 0u ? 127u : max(amax >> 23, 2u) - 2u;
    const float inv = __uint_as_float((254u - e) << 23);
    f2 m[4];
    float s0 = 0.0f, s1 = 0.0f;
    if (RULE == AWQ_MXFP4_MSE) {
        f2 m1[4];
        round8<true>(wp, inv, m, s0);
        round8<true>(wp, inv * 0.5f, m1, s1);
        const bool up = 4.0f * grp_sum<4>(s1) < grp_sum<4>(s0);
#pragma unroll
        for (int i = 0; i < 4; ++i) m[i] = up ? m1[i] : m[i];
        e += up ? 1u : 0u;
    } else {
        const bool up = RULE == AWQ_MXFP4_CEIL && __uint_as_float(amax) * inv > 6.0f;
        e += up ? 1u : 0u;
        round8<false>(wp, up ? inv * 0.5f : inv, m, s0);
    }
    const float scale = fp4_scale(e);
    f2 dq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f2 a = m[i] * (f2){scale, scale};                        // exact
        dq[i] = (f2){__uint_as_float(__float_as_uint(a.x) | (__float_as_uint(wp[i].x) & 0x80000000u)),
                     __uint_as_float(__float_as_uint(a.y) | (__float_as_uint(wp[i].y) & 0x80000000u))};
    }
    auto sum = [&](auto markstein) {
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f2 q;
            if constexpr (decltype(markstein)::value)
                q = (f2){mquot(dq[i].x, s[i].x, rs[i].x), mquot(dq[i].y, s[i].y, rs[i].y)};
            else
                q = (f2){dq[i].x / s[i].x, dq[i].y / s[i].y};
            const f2 d = q - w[i];
            const f2 c = xs[i] * (d * d);
            acc = acc + c.x;
            acc = acc + c.y;
        }
        return acc;
    };
    float acc = __builtin_nanf("");
    if (RT && e - 87u <= 80u) acc = sum(std::true_type{});
    if (__builtin_expect(!bad && acc != acc, 0)) acc = sum(std::false_type{});
    return acc;
}

template <typename F, int RULE, bool RT>
__global__ __launch_bounds__(256) void mxfp4_act_loss_kernel(const void* __restrict__ w, int64_t rows, int64_t K,
                                                             const float* __restrict__ table,
                                                             const float* __restrict__ rtable, int n_grid,
                                                             const float* __restrict__ x_sq, float* __restrict__ part,
                                                             int64_t stride) {
    extern __shared__ __attribute__((aligned(16))) float lds[];   // [candidate][scale row | reciprocal row][256]
    constexpr int kRowFloats = (RT ? 2 : 1) * kSlabCols;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * kSlabCols;           // the slab's first column
    const int lc = (lane & 31) * 8;                               // the lane's first column in the slab
    const int64_t col = c0 + lc;
    const bool cok = col < K;                                     // K % 32 == 0: true or false for a whole quad
    const int64_t nb = K / kBlockElems;

    f2 xs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xs[i] = (f2){0.0f, 0.0f};
    if (cok) {
        const f4v a = *(const f4v*)(x_sq + col), b = *(const f4v*)(x_sq + col + 4);
        xs[0] = (f2){a.x, a.y}; xs[1] = (f2){a.z, a.w}; xs[2] = (f2){b.x, b.y}; xs[3] = (f2){b.z, b.w};
    }

    for (int i0 = 0; i0 < n_grid; i0 += kCandChunk) {
        const int nc = min(kCandChunk, n_grid - i0);
        if (i0) __syncthreads();                                  // the previous chunk's reads are done
        for (int o = tid; o < nc * kRowFloats; o += 256) {
            const int c = o / kRowFloats, k = o % kRowFloats;
            const int64_t g = c0 + (k & (kSlabCols - 1));
            const float* src = (RT && k >= kSlabCols) ? rtable : table;
            lds[o] = g < K ? src[(int64_t)(i0 + c) * K + g] : 1.0f;
        }
        __syncthreads();

        for (int64_t r0 = (int64_t)blockIdx.y * kTripRows; r0 < rows; r0 += (int64_t)gridDim.y * kTripRows) {
            f2 wv[2][4];
            bool ok[2];
            int64_t blk[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t row = r0 + wave * 4 + j * 2 + (lane >> 5);
                ok[j] = cok && row < rows;
                blk[j] = row * nb + col / kBlockElems;
                Chunk<F::NW> ch;
#pragma unroll
                for (int h = 0; h < F::NW; ++h) {
                    ch.w[h] = (u4){0u, 0u, 0u, 0u};
                    if (ok[j])
                        ch.w[h] = __builtin_nontemporal_load((const u4*)((const char*)w + (row * K + col) * F::kBytes) + h);
                }
                chunk_pairs<F>(ch, wv[j]);
            }
            for (int i = 0; i < nc; ++i) {
                const f4v* row = (const f4v*)(lds + i * kRowFloats + lc);
                const f4v sa = row[0], sb = row[1];
                const f2 s[4] = {{sa.x, sa.y}, {sa.z, sa.w}, {sb.x, sb.y}, {sb.z, sb.w}};
                f2 rs[4] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
                if (RT) {
                    const f4v ra = row[kSlabCols / 4], rb = row[kSlabCols / 4 + 1];
                    rs[0] = (f2){ra.x, ra.y}; rs[1] = (f2){ra.z, ra.w}; rs[2] = (f2){rb.x, rb.y}; rs[3] = (f2){rb.z, rb.w};
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    bool bad;
                    const float own = lane_loss<F, RULE, RT>(wv[j], s, rs, xs, bad);
                    const float loss = grp_sum<4>(own);
                    if (ok[j] && (lane & 3) == 0)
                        part[(int64_t)(i0 + i) * stride + blk[j]] = bad ? __builtin_nanf("") : loss;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// awq_mxfp4.hip's quantize kernel with the column scale applied in registers.
// ---------------------------------------------------------------------------------------
template <typename F, int RULE>
__global__ __launch_bounds__(64) void mxfp4_quant_scaled_kernel(const void* __restrict__ x,
                                                                const float* __restrict__ col_scale,
                                                                uint8_t* __restrict__ codes,
                                                                uint8_t* __restrict__ scales, int64_t n_elems,
                                                                int64_t K, int64_t tiles) {
    const int lane = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t e0 = tile * kTileElems;
        const uint32_t te = (uint32_t)min((int64_t)kTileElems, n_elems - e0);   // elements of this segment
        const __amdgpu_buffer_rsrc_t rx = rsrc((const char*)x + e0 * F::kBytes, te * (uint32_t)F::kBytes);
        const __amdgpu_buffer_rsrc_t rc = rsrc(codes + e0 / 2, te / 2u);
        const int64_t k0 = e0 % K;                                              // the segment's first column
        Chunk<F::NW> v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int h = 0; h < F::NW; ++h)
                v[j].w[h] = __builtin_amdgcn_raw_buffer_load_b128(
                    rx, (uint32_t)(j * 512 * F::kBytes + lane * 8 * F::kBytes + 16 * h), 0, AWQ_LOAD_AUX);

        uint32_t eb[4], sd = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // the lane's column: below K always (K % 8 == 0, so its 8 elements share a row)
            int64_t k = k0 + j * 512 + lane * 8;
            if (K >= kTileElems) k -= k >= K ? K : 0;
            else k = (int64_t)((uint32_t)k % (uint32_t)K);
            const f4v sa = *(const f4v*)(col_scale + k), sb = *(const f4v*)(col_scale + k + 4);
            const f2 s[4] = {{sa.x, sa.y}, {sa.z, sa.w}, {sb.x, sb.y}, {sb.z, sb.w}};
            f2 wv[4];
            chunk_pairs<F>(v[j], wv);
            float y[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f2 p = scale_pair<F>(wv[i], s[i]);
                y[2 * i] = p.x;
                y[2 * i + 1] = p.y;
            }
            uint32_t word;
            eb[j] = mxfp4_block<F, RULE>(make_chunk<F>(y), word);
            __builtin_amdgcn_raw_buffer_store_b32(word, rc, (uint32_t)(j * 256 + lane * 4), 0, AWQ_STORE_AUX);
            gather_scale_bytes(eb[j], lane, j, sd);
        }
        store_scale_bytes(scales + e0 / kBlockElems, te, lane, sd, eb);
    }
}

template <typename F, bool RT>
void launch_loss(int rule, dim3 grid, size_t lds_bytes, hipStream_t st, const void* w, int64_t rows, int64_t K,
                 const float* table, const float* rtable, int n_grid, const float* x_sq, float* part, int64_t stride) {
#define AWQ_MX(R)                                                                                            \
    hipLaunchKernelGGL((mxfp4_act_loss_kernel<F, R, RT>), grid, dim3(256), lds_bytes, st, w, rows, K, table, \
                       rtable, n_grid, x_sq, part, stride)
    if (rule == AWQ_MXFP4_FLOOR) AWQ_MX(AWQ_MXFP4_FLOOR);
    else if (rule == AWQ_MXFP4_CEIL) AWQ_MX(AWQ_MXFP4_CEIL);
    else AWQ_MX(AWQ_MXFP4_MSE);
#undef AWQ_MX
}

template <typename F>
void launch_quant_scaled(int rule, unsigned grid, hipStream_t st, const void* x, const float* col_scale,
                         uint8_t* codes, uint8_t* scales, int64_t n, int64_t K, int64_t tiles) {
#define AWQ_MX(R)                                                                                           \
    hipLaunchKernelGGL((mxfp4_quant_scaled_kernel<F, R>), dim3(grid), dim3(64), 0, st, x, col_scale, codes, \
                       scales, n, K, tiles)
    if (rule == AWQ_MXFP4_FLOOR) AWQ_MX(AWQ_MXFP4_FLOOR);
    else if (rule == AWQ_MXFP4_CEIL) AWQ_MX(AWQ_MXFP4_CEIL);
    else AWQ_MX(AWQ_MXFP4_MSE);
#undef AWQ_MX
}

}  // namespace
}  // namespace awq

using namespace awq;

extern "C" int awq_act_search_losses_mxfp4(const void* w, int dtype, int64_t rows, int64_t K, int rule,
                                           const float* table, const float* rtable, int n_grid, const float* x_sq,
                                           float* part, int64_t part_stride, void* stream) {
    const char* const what = "awq_act_search_losses_mxfp4";
    if (int rc = check_common(what, dtype, rows, K)) return rc;
    if (!mxfp4_rule_ok(rule))
        return fail(AWQ_EINVAL, "%s: scale rule %d is not floor (0), ceil (1) or mse (2)", what, rule);
    if (n_grid < 1 || n_grid > AWQ_ACT_MAX_GRID)
        return fail(AWQ_EINVAL, "%s: n_grid must be in [1, %d] (got %d)", what, AWQ_ACT_MAX_GRID, n_grid);
    const int64_t n = rows * K;
    if (n == 0) return AWQ_OK;
    if (part_stride < n / kBlockElems)
        return fail(AWQ_EINVAL, "%s: part_stride %lld is smaller than the %lld blocks", what, (long long)part_stride,
                    (long long)(n / kBlockElems));
    const int64_t slabs = (K + kSlabCols - 1) / kSlabCols;
    if (slabs > (int64_t)0x7FFFFFFF)
        return fail(AWQ_EUNSUPPORTED, "%s: K %lld is beyond the grid's 2^31 - 1 column slabs", what, (long long)K);
    if (!w || !table || !x_sq || !part) return fail(AWQ_EINVAL, "%s: null argument", what);
    if (!aligned(w, 16) || !aligned(table, 16) || !aligned(rtable, 16) || !aligned(x_sq, 16) || !aligned(part, 4))
        return fail(AWQ_EINVAL, "%s: w, table, rtable and x_sq need 16-B alignment, part 4-B", what);
    hipStream_t st = (hipStream_t)stream;
    const int64_t trips = (rows + kTripRows - 1) / kTripRows;
    const unsigned gy = diag_cap((unsigned)std::min<int64_t>(
        std::min<int64_t>(trips, 65535), std::max<int64_t>(1, kLossGroups / slabs)));
    const dim3 grid((unsigned)slabs, gy);
    const size_t lds = (size_t)std::min(n_grid, kCandChunk) * (rtable ? 2 : 1) * kSlabCols * sizeof(float);
#define AWQ_MX(F)                                                                                              \
    do {                                                                                                       \
        if (rtable) launch_loss<F, true>(rule, grid, lds, st, w, rows, K, table, rtable, n_grid, x_sq, part, part_stride); \
        else launch_loss<F, false>(rule, grid, lds, st, w, rows, K, table, rtable, n_grid, x_sq, part, part_stride);       \
    } while (0)
    if (dtype == AWQ_DTYPE_BF16) AWQ_MX(FmtBF16);
    else if (dtype == AWQ_DTYPE_F16) AWQ_MX(FmtF16);
    else AWQ_MX(FmtF32);
#undef AWQ_MX
    return hip_status(hipPeekAtLastError(), "awq mxfp4 act loss kernel");
}

extern "C" int awq_quantize_mxfp4_scaled(const void* w, int dtype, int64_t rows, int64_t K, int rule,
                                         const float* col_scale, uint8_t* codes, uint8_t* scales, void* stream) {
    const char* const what = "awq_quantize_mxfp4_scaled";
    if (int rc = check_common(what, dtype, rows, K)) return rc;
    if (!mxfp4_rule_ok(rule))
        return fail(AWQ_EINVAL, "%s: scale rule %d is not floor (0), ceil (1) or mse (2)", what, rule);
    const int64_t n = rows * K;
    if (n == 0) return AWQ_OK;
    if (!w || !col_scale || !codes || !scales) return fail(AWQ_EINVAL, "%s: null argument", what);
    if (!aligned(w, 16) || !aligned(col_scale, 16) || !aligned(codes, 4) || !aligned(scales, 4))
        return fail(AWQ_EINVAL, "%s: w and col_scale need 16-B alignment, codes and scales 4-B", what);
    hipStream_t st = (hipStream_t)stream;
    const int64_t tiles = (n + kTileElems - 1) / kTileElems;
    const unsigned grid = diag_cap((unsigned)std::min<int64_t>(tiles, kQuantWaves));
    if (dtype == AWQ_DTYPE_BF16) launch_quant_scaled<FmtBF16>(rule, grid, st, w, col_scale, codes, scales, n, K, tiles);
    else if (dtype == AWQ_DTYPE_F16) launch_quant_scaled<FmtF16>(rule, grid, st, w, col_scale, codes, scales, n, K, tiles);
    else launch_quant_scaled<FmtF32>(rule, grid, st, w, col_scale, codes, scales, n, K, tiles);
    return hip_status(hipPeekAtLastError(), "awq mxfp4 scaled quantize kernel");
}
