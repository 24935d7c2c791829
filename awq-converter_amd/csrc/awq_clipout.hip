// awq_clipout.hip — clip search with the token-sample loss (awq_quantize_clip_output,
// include/awq_hip.h): awq_quantize_clip_scaled's candidates and packed outputs,
// each (row, group, candidate) scored by the error at the linear's output on samples X [T, K],
//   E[t] = sum_{k in group} d[k] x[t, k],  loss = sum_t E[t]^2,
// the published per-group clip objective (AutoAWQ _compute_best_clip).  Self-contained: the entry
// points, their validation and the two kernels.
//
// Per element the arithmetic is awq_actclip.hip's chunk_loss up to d (w' = RN_D(w s), q of w',
// dq = fp16(fp16(q - z) fp16(scale)), d = RN_f32(dq / s) - w) through the same awq_quant.h helpers
// (group_range, params_from_range, F::quot, quant8_fast / quant8_special), so a candidate's packed
// bits are awq_quantize_clip_scaled's; the product with X is awq_outerr.hip's (hi / lo bf16 split,
// v_mfma_f32_32x32x16_bf16, the NT lane maps).  The sums over k are in the implementation's order:
// the contract is §5.13's bound with the group size for K.  No floating-point atomics: one lane
// forms a (row, group, candidate) loss, the tokens in a fixed order.
//   * fast (bf16, group_size 32 / 64 / 128 / 256, 16-B aligned w / x / col_scale, x_row_stride %
//     8 == 0): a workgroup of 4 waves takes 128 rows of one group; the group's w stays in registers
//     (lane (r, h) holds row r's 8 k of every 16-k step), candidates are the outer loop, the X
//     slice goes through LDS in token chunks shared by the four waves;
//   * generic (everything else the entry accepts): one wave per group, d through LDS, one token
//     per lane with the k in ascending order on f32 operands.  Correct, not fast.
// A group's zero-point field is OR-ed into qzeros, which the launcher zeroes first (integer
// atomics: order-free).
#include <algorithm>

#include "awq_quant.h"

namespace awq {
namespace {

typedef __bf16 bf8v __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kRowTile = 128;                      // fast kernel: rows per workgroup (4 waves x 32)
constexpr int64_t kMaxDesc = (int64_t)1 << 22;     // fast kernel: K and x_row_stride below this keep a
                                                   // tile's buffer ranges and offsets below 2^31
constexpr int64_t kMaxProduct = (int64_t)1 << 60;

// tokens per LDS chunk of the fast kernel: 128, or 64 at group_size 256 (the chunk stays under
// 36 KiB: [tokens][group_size + 8] bf16)
__host__ __device__ constexpr int chunk_tokens(int gs) { return gs <= 128 ? 128 : 64; }

struct OutArgs {
    const void* w;
    const float* cs;
    const float* rs;       // or nullptr
    const void* x;
    int32_t* qweight;
    int32_t* qzeros;
    uint16_t* scales;
    int32_t* best_idx;
    float* gloss;          // [2, loss_stride] or nullptr
    float* closs;          // [n_cand, loss_stride] or nullptr
    int64_t loss_stride;
    int64_t rows, K, T, xs;
    int n_grid, c0, n_cand;
    uint32_t nan_code;
};

// w' = RN_D(RN_f32(w s[k])) (awq_apply_input_scale)
template <typename F>
__device__ __forceinline__ void scaled8(const float (&w)[8], const float (&cs)[8], float (&y)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = F::rn(opaque(w[i] * cs[i]));
}

// One candidate's d over a lane's 8 elements: q (awq.py:245-248) of w' = y, dq = fp16(fp16(q - z) *
// fp16(scale)) (awq.py:459-539), d = RN_f32(dq / s[k]) - w.  ieee: the IEEE division, else the
// quotient through the reciprocals (a NaN wherever a reciprocal is out of range: the caller redoes
// the candidate).
template <typename F, int BITS, bool SYM>
__device__ __forceinline__ void chunk_d(const float (&w)[8], const float (&y)[8], const float (&cs)[8],
                                        const float (&rs)[8], bool ieee, const GroupParams& p, float (&d)[8]) {
    constexpr float QMIN = SYM ? -(float)(1 << (BITS - 1)) : 0.0f;
    constexpr float QMAX = SYM ? (float)((1 << (BITS - 1)) - 1) : (float)((1 << BITS) - 1);
    const float zf = F::as_fmt(p.z);
    const float sh = F::dq_scale(p.s);
    const bool special = !F::fast(p.r);   // scale 0 / inf / NaN: exact division, NaN-propagating clamp
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float x = y[i];
        float q;
        if (__builtin_expect(special, 0)) {
            const float t = F::rn(opaque(x) / p.s);
            const float rr = __builtin_rintf(SYM ? t : F::rn(t + zf));
            q = __builtin_isnan(rr) ? rr : __builtin_fminf(__builtin_fmaxf(rr, QMIN), QMAX);
        } else {
            const float t = F::quot(x, p.s, p.r);
            q = __builtin_fminf(__builtin_fmaxf(__builtin_rintf(SYM ? t : F::rn(t + zf)), QMIN), QMAX);
        }
        // q - z is an integer of magnitude <= 510 (exact in fp16); the product of two fp16 values
        // is exact in fp32, so the conversion is the fp16 multiply's single rounding
        d[i] = (float)(_Float16)opaque((q - zf) * sh);
    }
    if (ieee) {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = d[i] / cs[i] - w[i];
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = mquot(d[i], cs[i], rs[i]) - w[i];
    }
}

// The running winner of one group: the first strict minimum of the losses as stored.
struct Pick {
    float best, first;
    int bi;
    __device__ void start(int c0) { best = __builtin_inff(); first = 0.0f; bi = c0; }
    __device__ void take(int c, int c0, float e) {
        if (c == c0) first = e;
        if (e < best) { best = e; bi = c; }
    }
};

// per-group scalars and the zero-point field, written by one lane of the group (fg = r G + g)
template <int BITS, bool SYM>
__device__ __forceinline__ void store_group(const OutArgs& a, int64_t fg, int64_t zword, int zslot,
                                            const GroupParams& p, bool gnan, int best, float first, float lossw) {
    if (a.scales) a.scales[fg] = f16_bits(p.s, gnan, a.nan_code);
    if (a.best_idx) a.best_idx[fg] = best;
    if (a.gloss) {
        a.gloss[fg] = first;
        a.gloss[a.loss_stride + fg] = lossw;
    }
    if (a.qzeros) atomicOr((unsigned int*)a.qzeros + zword, zero_field<BITS, SYM>(p.z) << (BITS * zslot));
}

// ---------------------------------------------------------------------------------------
// Fast kernel.  Tile = (128-row block, group).  Wave v owns rows 32 v .. 32 v + 31; lane l
// (r = l & 31, h = l >> 5) holds A[row r][k = 16 s + 8 h + j] of every 16-k step s: one 16-B load
// of w per step, kept across the candidate loop.  The group's col_scale and reciprocals sit in
// LDS.  Per candidate every lane forms the parameters, d of its 8 k of every step split into
// d_hi = RN_bf16(d), d_lo = RN_bf16(d - d_hi), and then walks the tokens: chunks of CT tokens of
// the group's X slice in LDS ([CT][GS + 8] bf16, staged by all four waves; re-staged per candidate
// only when T > CT), 32-token tiles inside a chunk — one accumulator, 2 GS / 16 MFMAs, B[k = 8 h +
// j][col r] one 16-B LDS read per two MFMAs — whose 16 values (token 32 j + r, row (i & 3) + 8 (i
// >> 2) + 4 h) are squared into 16 running sums.  After the last chunk the sums are added over the
// half's 32 lanes (the butterfly: a fixed order) and each lane picks its own row's, from its half
// or the other.  Rows and tokens past the end read zeros (buffer descriptors) and store nothing.
// ---------------------------------------------------------------------------------------
template <int BITS, bool SYM, int GS>
__global__ __launch_bounds__(256) void clipout_mfma_kernel(OutArgs a, int64_t tiles) {
    typedef FmtBF16 F;
    constexpr int NS = GS / 16, CT = chunk_tokens(GS), XROW = (GS + 8) * 2, XBYTES = CT * XROW, PER = 32 / BITS;
    constexpr int PIECES = CT * (GS / 8);
    __shared__ __attribute__((aligned(16))) char lds[XBYTES + 2 * GS * 4];
    float* const lcs = (float*)(lds + XBYTES);
    float* const lrs = lcs + GS;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
    const int64_t G = a.K / GS, zpr = (G + PER - 1) / PER;
    const uint32_t Ku = (uint32_t)a.K, xsu = (uint32_t)a.xs;
    const bool have_rs = a.rs != nullptr;
    const int64_t n_chunks = (a.T + CT - 1) / CT;
    const uint32_t row = 32u * wv + r;
    const int sel = (r & 3) + 4 * (r >> 3);        // the accumulator register of row r ...
    const bool sel_hi = ((r >> 2) & 1) != 0;       // ... in this half of the wave

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t rb = tile / G, g = tile - rb * G;
        const int64_t n0 = rb * kRowTile;
        const uint32_t nn = (uint32_t)min((int64_t)kRowTile, a.rows - n0);
        const bool row_ok = row < nn;
        const int64_t grow = n0 + row;
        const __amdgpu_buffer_rsrc_t rw = rsrc((const char*)a.w + (n0 * a.K + g * GS) * 2, ((nn - 1u) * Ku + GS) * 2u);

        // chunk ch of the group's X slice -> LDS: piece c = token c / (GS / 8), k 8 (c % (GS / 8))
        auto stage = [&](int64_t ch) {
            const int64_t t0 = ch * CT;
            const uint32_t tn = (uint32_t)min((int64_t)CT, a.T - t0);
            const __amdgpu_buffer_rsrc_t rx = rsrc((const char*)a.x + (t0 * a.xs + g * GS) * 2, ((tn - 1u) * xsu + GS) * 2u);
            u4 xr[PIECES / 256];
#pragma unroll
            for (int i = 0; i < PIECES / 256; ++i) {
                const uint32_t c = (uint32_t)tid + 256u * i;
                xr[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, ((c / (GS / 8)) * xsu + 8u * (c % (GS / 8))) * 2u, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < PIECES / 256; ++i) {
                const uint32_t c = (uint32_t)tid + 256u * i;
                *(u4*)(lds + (c / (GS / 8)) * XROW + (c % (GS / 8)) * 16u) = xr[i];
            }
        };

        __syncthreads();                          // the previous tile's readers are done
        if (tid < GS) {
            lcs[tid] = a.cs[g * GS + tid];
            lrs[tid] = have_rs ? a.rs[g * GS + tid] : 0.0f;
        }
        u4 wr[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s)
            wr[s] = __builtin_amdgcn_raw_buffer_load_b128(rw, (row * Ku + 16u * s + 8u * h) * 2u, 0, 0);
        if (n_chunks == 1) stage(0);              // one chunk: staged once per tile, not per candidate
        __syncthreads();

        // a step's 8 weights, column scales and reciprocals
        auto step_in = [&](int s, float (&w)[8], float (&cs)[8], float (&rs)[8]) {
            Chunk<1> v;
            v.w[0] = wr[s];
            const f4v c0 = *(const f4v*)(lcs + 16 * s + 8 * h), c1 = *(const f4v*)(lcs + 16 * s + 8 * h + 4);
            const f4v r0 = *(const f4v*)(lrs + 16 * s + 8 * h), r1 = *(const f4v*)(lrs + 16 * s + 8 * h + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                cs[i] = c0[i]; cs[4 + i] = c1[i];
                rs[i] = r0[i]; rs[4 + i] = r1[i];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = F::elem(v, i);
        };

        // the group's [mn, mx] of w' from the raw bits: the steps in registers, then the other half
        int sm = INT32_MIN;
        uint32_t um = 0, cm = 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float w[8], cs[8], rs[8], y[8];
            step_in(s, w, cs, rs);
            scaled8<F>(w, cs, y);
            const Chunk<1> v = make_chunk<F>(y);
            int s1;
            uint32_t u1;
            F::lane_max(v, s1, u1);
            sm = max(sm, s1);
            um = max(um, u1);
            cm = max(cm, F::lane_cmax(v));
        }
        {
            int p, q;
            swap32(sm, p, q);
            sm = max(p, q);
            uint32_t e, f;
            swap32(um, e, f);
            um = max(e, f);
            swap32(cm, e, f);
            cm = max(e, f);
        }
        float gmn, gmx;
        bool gnan;
        group_range<F, SYM>(sm, um, F::kOnes - cm, gmn, gmx, gnan);

        Pick pick;
        pick.start(a.c0);
        for (int c = a.c0; c < a.c0 + a.n_cand; ++c) {
            const float al = clip_alpha(a.n_grid, c);
            const GroupParams cp = params_from_range<F, BITS, SYM>(clip_shrink<F>(gmn, al), clip_shrink<F>(gmx, al));
            u4 fhi[NS], flo[NS];
            bool ieee = !have_rs;
            for (;;) {
                bool bad = false;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    float w[8], cs[8], rs[8], y[8], d[8];
                    step_in(s, w, cs, rs);
                    scaled8<F>(w, cs, y);
                    chunk_d<F, BITS, SYM>(w, y, cs, rs, ieee, cp, d);
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float d0 = d[2 * t], d1 = d[2 * t + 1];
                        bad = bad || d0 != d0 || d1 != d1;
                        const uint32_t hb = __builtin_bit_cast(uint32_t, __builtin_convertvector((f2){d0, d1}, b2));
                        const float l0 = d0 - __uint_as_float(hb << 16), l1 = d1 - __uint_as_float(hb & 0xFFFF0000u);
                        fhi[s][t] = hb;
                        flo[s][t] = __builtin_bit_cast(uint32_t, __builtin_convertvector((f2){l0, l1}, b2));
                    }
                }
                // a NaN d (an out-of-range reciprocal is NaN): the wave redoes the candidate with
                // IEEE divisions — the same bits wherever the quotient is exact
                if (ieee || __builtin_amdgcn_ballot_w64(bad) == 0) break;
                ieee = true;
            }

            float sq[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) sq[i] = 0.0f;
            for (int64_t ch = 0; ch < n_chunks; ++ch) {
                if (n_chunks > 1) {
                    __syncthreads();
                    stage(ch);
                    __syncthreads();
                }
                const uint32_t tn = (uint32_t)min((int64_t)CT, a.T - ch * CT);
                for (uint32_t j = 0; j < (uint32_t)(CT / 32) && 32u * j < tn; ++j) {
                    f16v acc;
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const bf8v xb = __builtin_bit_cast(bf8v, *(const u4*)(lds + (32u * j + r) * XROW + (16 * s + 8 * h) * 2));
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8v, fhi[s]), xb, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8v, flo[s]), xb, acc, 0, 0, 0);
                    }
                    const bool in = 32u * j + r < tn;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float e = acc[i];
                        sq[i] = sq[i] + (in ? e * e : 0.0f);
                    }
                }
            }
            float mine = 0.0f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float v = grp_sum<32>(sq[i]);
                if (i == sel) mine = v;
            }
            float lo_half, hi_half;
            swap32(mine, lo_half, hi_half);
            const float e = sel_hi ? hi_half : lo_half;
            if (a.closs && row_ok && h == 0) a.closs[(int64_t)(c - a.c0) * a.loss_stride + grow * G + g] = e;
            pick.take(c, a.c0, e);
        }

        const int best = gnan ? a.c0 : pick.bi;
        if (!gnan && best != 0) {
            const float al = clip_alpha(a.n_grid, best);
            gmn = clip_shrink<F>(gmn, al);
            gmx = clip_shrink<F>(gmx, al);
        }
        const GroupParams p = params_from_range<F, BITS, SYM>(gmn, gmx);
        if (a.qweight) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                float w[8], cs[8], rs[8], y[8];
                step_in(s, w, cs, rs);
                scaled8<F>(w, cs, y);
                const u2v word = pack_winner<F, BITS, SYM>(make_chunk<F>(y), p);
                if (row_ok) {
                    int32_t* qw = a.qweight + (grow * a.K + g * GS + 16 * s + 8 * h) / 8 * (BITS / 4);
                    qw[0] = (int32_t)word.x;
                    if (BITS == 8) qw[1] = (int32_t)word.y;
                }
            }
        }
        if (row_ok && h == 0)
            store_group<BITS, SYM>(a, grow * G + g, grow * zpr + g / PER, (int)(g % PER), p, gnan, best, pick.first,
                                   best == a.c0 ? pick.first : pick.best);
    }
}

// ---------------------------------------------------------------------------------------
// Generic kernel: one wave per group (a grid-stride loop over the flat groups).  Lane c < gs / 8
// holds chunk c, loaded element by element (pointers only element-aligned); the range reductions
// are whole-wave butterflies (lanes past the group repeat its last chunk).  Per candidate the
// lanes' d go to LDS, then lane l takes tokens l, l + 64, ...: E = the k in ascending order from
// +0 on f32 operands (one multiply, one add per k, no contraction), E^2 added in token order; the
// wave's 64 sums meet in the xor butterfly.
// ---------------------------------------------------------------------------------------
template <typename F, int BITS, bool SYM>
__global__ __launch_bounds__(64) void clipout_generic_kernel(OutArgs a, int gs) {
    constexpr int PER = 32 / BITS;
    typedef typename std::conditional<F::NW == 2, uint32_t, uint16_t>::type E;
    __shared__ float ds[512];
    const int lane = threadIdx.x;
    const int64_t G = a.K / gs, zpr = (G + PER - 1) / PER, total = a.rows * G;
    const int nch = gs / 8;
    const bool active = lane < nch;
    const int ch = active ? lane : nch - 1;   // lanes past the group repeat its last chunk
    for (int64_t fg = blockIdx.x; fg < total; fg += gridDim.x) {
        const int64_t r = fg / G, g = fg - r * G;
        const int64_t k0 = g * gs + 8 * ch;
        const E* src = (const E*)a.w + r * a.K + k0;
        float w[8], cs[8], rs[8], y[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            w[i] = F::dec(src[i]);
            cs[i] = a.cs[k0 + i];
            rs[i] = 0.0f;
        }
        scaled8<F>(w, cs, y);
        const Chunk<F::NW> v = make_chunk<F>(y);
        int sm;
        uint32_t um;
        F::lane_max(v, sm, um);
        const int smax = wave_max_up(sm);
        const uint32_t umax = wave_max_up(um);
        const uint32_t umin = F::kOnes - wave_max_up(F::lane_cmax(v));
        float gmn, gmx;
        bool gnan;
        group_range<F, SYM>(smax, umax, umin, gmn, gmx, gnan);

        Pick pick;
        pick.start(a.c0);
        for (int c = a.c0; c < a.c0 + a.n_cand; ++c) {
            const float al = clip_alpha(a.n_grid, c);
            const GroupParams cp = params_from_range<F, BITS, SYM>(clip_shrink<F>(gmn, al), clip_shrink<F>(gmx, al));
            float d[8];
            chunk_d<F, BITS, SYM>(w, y, cs, rs, true, cp, d);
            __syncthreads();                      // the previous candidate's readers are done
            if (active) {
#pragma unroll
                for (int i = 0; i < 8; ++i) ds[8 * lane + i] = d[i];
            }
            __syncthreads();
            float sq = 0.0f;
            for (int64_t t = lane; t < a.T; t += 64) {
                const E* xr = (const E*)a.x + t * a.xs + g * gs;
                float e = 0.0f;
                for (int k = 0; k < gs; ++k) e = e + ds[k] * F::dec(xr[k]);
                sq = sq + e * e;
            }
            const float e = wave_sum(sq);
            if (a.closs && lane == 0) a.closs[(int64_t)(c - a.c0) * a.loss_stride + fg] = e;
            pick.take(c, a.c0, e);
        }

        const int best = gnan ? a.c0 : pick.bi;
        if (!gnan && best != 0) {
            const float al = clip_alpha(a.n_grid, best);
            gmn = clip_shrink<F>(gmn, al);
            gmx = clip_shrink<F>(gmx, al);
        }
        const GroupParams p = params_from_range<F, BITS, SYM>(gmn, gmx);
        if (a.qweight) {
            const u2v word = pack_winner<F, BITS, SYM>(v, p);
            if (active) {
                int32_t* qw = a.qweight + (r * a.K + k0) / 8 * (BITS / 4);
                qw[0] = (int32_t)word.x;
                if (BITS == 8) qw[1] = (int32_t)word.y;
            }
        }
        if (lane == 0)
            store_group<BITS, SYM>(a, fg, r * zpr + g / PER, (int)(g % PER), p, gnan, best, pick.first,
                                   best == a.c0 ? pick.first : pick.best);
    }
}

template <int BITS, bool SYM>
void launch_mfma(int gs, unsigned grid, hipStream_t st, const OutArgs& a, int64_t tiles) {
    switch (gs) {
    case 32: hipLaunchKernelGGL((clipout_mfma_kernel<BITS, SYM, 32>), dim3(grid), dim3(256), 0, st, a, tiles); break;
    case 64: hipLaunchKernelGGL((clipout_mfma_kernel<BITS, SYM, 64>), dim3(grid), dim3(256), 0, st, a, tiles); break;
    case 128: hipLaunchKernelGGL((clipout_mfma_kernel<BITS, SYM, 128>), dim3(grid), dim3(256), 0, st, a, tiles); break;
    default: hipLaunchKernelGGL((clipout_mfma_kernel<BITS, SYM, 256>), dim3(grid), dim3(256), 0, st, a, tiles); break;
    }
}

template <typename F>
void launch_generic(int gs, int bits, int sym, unsigned grid, hipStream_t st, const OutArgs& a) {
    switch ((bits == 8 ? 2 : 0) + (sym ? 1 : 0)) {
    case 0: hipLaunchKernelGGL((clipout_generic_kernel<F, 4, false>), dim3(grid), dim3(64), 0, st, a, gs); break;
    case 1: hipLaunchKernelGGL((clipout_generic_kernel<F, 4, true>), dim3(grid), dim3(64), 0, st, a, gs); break;
    case 2: hipLaunchKernelGGL((clipout_generic_kernel<F, 8, false>), dim3(grid), dim3(64), 0, st, a, gs); break;
    default: hipLaunchKernelGGL((clipout_generic_kernel<F, 8, true>), dim3(grid), dim3(64), 0, st, a, gs); break;
    }
}

}  // namespace
}  // namespace awq

using namespace awq;

// the one predicate of the fast kernel: the entry routes by it, the tests ask it
extern "C" int awq_quantize_clip_output_fast(const void* w, int dtype, int64_t K, int64_t group_size,
                                             const float* col_scale, const float* col_rscale, const void* x,
                                             int64_t x_row_stride) {
    return dtype == AWQ_DTYPE_BF16 && fast_group_size(group_size) && K > 0 && K % group_size == 0 && aligned(w, 16) &&
           aligned(x, 16) && aligned(col_scale, 16) && aligned(col_rscale, 16) && x_row_stride >= K &&
           x_row_stride % 8 == 0 && K < kMaxDesc && x_row_stride < kMaxDesc;
}

extern "C" int64_t awq_quantize_clip_output_work_bytes(int64_t rows, int64_t K, int64_t group_size, int64_t T,
                                                       int n_candidates) {
    (void)rows; (void)K; (void)group_size; (void)T; (void)n_candidates;
    return 0;   // every loss is formed in registers: no workspace
}

extern "C" int awq_quantize_clip_output(const void* w, int dtype, int64_t rows, int64_t K, int64_t group_size, int bits,
                                        int symmetric, const float* col_scale, const float* col_rscale, const void* x,
                                        int64_t T, int64_t x_row_stride, int n_grid, int cand_begin, int n_candidates,
                                        int32_t* qweight, int32_t* qzeros, uint16_t* scales, int32_t* best_idx,
                                        float* group_loss, float* cand_loss, int64_t loss_stride, void* work,
                                        void* stream) {
    (void)work;
    set_error(AWQ_OK, "");
    const long long gs = group_size, R = rows, KK = K;   // (long long: the messages' %lld)
    if (bits != 4 && bits != 8) return fail(AWQ_EINVAL, "Unsupported bit width: %d. Supported: 4, 8.", bits);
    if (gs <= 0) return fail(AWQ_EINVAL, "Group size must be a positive integer: %lld", gs);
    if (rows < 0 || K < 0 || T < 0) return fail(AWQ_EINVAL, "negative shape (%lld, %lld, %lld)", R, KK, (long long)T);
    if (gs < 8 || gs > 512 || (gs & (gs - 1)))
        return fail(AWQ_EUNSUPPORTED, "awq_quantize_clip_output: group_size %lld is not a power of two in [8, 512]", gs);
    if (K % gs)
        return fail(AWQ_EUNSUPPORTED, "awq_quantize_clip_output: K %lld is not a multiple of group_size %lld", KK, gs);
    if (dtype == AWQ_DTYPE_F64) return fail(AWQ_EUNSUPPORTED, "awq_quantize_clip_output: fp64 weights are not supported");
    if (dtype != AWQ_DTYPE_BF16 && dtype != AWQ_DTYPE_F16 && dtype != AWQ_DTYPE_F32)
        return fail(AWQ_EINVAL, "awq_quantize_clip_output: dtype code %d is not a weight dtype (bf16, fp16, fp32)", dtype);
    if (x_row_stride < K)
        return fail(AWQ_EINVAL, "awq_quantize_clip_output: x_row_stride %lld < K %lld", (long long)x_row_stride, KK);
    if (n_grid < 1 || n_candidates < 1 || cand_begin < 0 || n_candidates > n_grid - cand_begin)
        return fail(AWQ_EINVAL, "clip search needs 0 <= cand_begin (%d), 1 <= n_candidates (%d), their sum <= n_grid (%d)",
                    cand_begin, n_candidates, n_grid);
    const long long G = K / gs;
    if (rows > 0 && (K > kMaxProduct / rows || T > kMaxProduct / rows || (T > 0 && x_row_stride > kMaxProduct / T) ||
                     G > (int64_t)0x7FFFFFFF / rows))
        return fail(AWQ_EUNSUPPORTED, "awq_quantize_clip_output: %lld x %lld weights on %lld tokens exceed the kernels' range",
                    R, KK, (long long)T);
    if (!qweight && !qzeros && !scales && !best_idx && !group_loss && !cand_loss)
        return fail(AWQ_EINVAL, "no output requested");
    if (rows == 0 || K == 0) return AWQ_OK;   // empty: the pointers are not looked at
    if (!w || !col_scale || (T > 0 && !x)) return fail(AWQ_EINVAL, "awq_quantize_clip_output: null input");
    if ((group_loss || cand_loss) && loss_stride < rows * G)
        return fail(AWQ_EINVAL, "group_loss / cand_loss need loss_stride (%lld) >= rows * G (%lld)", (long long)loss_stride,
                    R * G);
    const size_t esz = dtype == AWQ_DTYPE_F32 ? 4 : 2;
    if (!aligned(w, esz) || !aligned(x, esz) || !aligned(col_scale, 4) || !aligned(col_rscale, 4) || !aligned(qweight, 4) ||
        !aligned(qzeros, 4) || !aligned(scales, 2) || !aligned(best_idx, 4) || !aligned(group_loss, 4) ||
        !aligned(cand_loss, 4))
        return fail(AWQ_EINVAL, "awq_quantize_clip_output: a pointer is not aligned to its element size");
    hipStream_t st = (hipStream_t)stream;
    OutArgs a;
    a.w = w; a.cs = col_scale; a.rs = col_rscale; a.x = x;
    a.qweight = qweight; a.qzeros = qzeros; a.scales = scales; a.best_idx = best_idx;
    a.gloss = group_loss; a.closs = cand_loss; a.loss_stride = loss_stride;
    a.rows = rows; a.K = K; a.T = T; a.xs = x_row_stride;
    a.n_grid = n_grid; a.c0 = cand_begin; a.n_cand = n_candidates;
    a.nan_code = nan_scale_code(dtype, symmetric, false);
    const int64_t C = 32 / bits, WPR = (G + C - 1) / C;
    hipError_t e = hipSuccess;
    // every group ORs its zero-point field into its word
    if (qzeros) e = hipMemsetAsync(qzeros, 0, (size_t)(rows * WPR) * 4, st);
    if (e == hipSuccess) {
        if (awq_quantize_clip_output_fast(w, dtype, K, group_size, col_scale, col_rscale, x, x_row_stride)) {
            const int64_t tiles = (rows + kRowTile - 1) / kRowTile * G;
            const unsigned grid = diag_cap((unsigned)std::min<int64_t>(tiles, 0x7FFFFFFF));
            switch ((bits == 8 ? 2 : 0) + (symmetric ? 1 : 0)) {
            case 0: launch_mfma<4, false>((int)gs, grid, st, a, tiles); break;
            case 1: launch_mfma<4, true>((int)gs, grid, st, a, tiles); break;
            case 2: launch_mfma<8, false>((int)gs, grid, st, a, tiles); break;
            default: launch_mfma<8, true>((int)gs, grid, st, a, tiles); break;
            }
        } else {
            const unsigned grid = diag_cap((unsigned)(rows * G));
            if (dtype == AWQ_DTYPE_BF16) launch_generic<FmtBF16>((int)gs, bits, symmetric, grid, st, a);
            else if (dtype == AWQ_DTYPE_F16) launch_generic<FmtF16>((int)gs, bits, symmetric, grid, st, a);
            else launch_generic<FmtF32>((int)gs, bits, symmetric, grid, st, a);
        }
        e = hipPeekAtLastError();
    }
    return hip_status(e, "awq clip-output kernels");
}
