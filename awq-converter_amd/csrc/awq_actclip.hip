// awq_actclip.hip — activation-aware clip search (awq_quantize_clip_scaled, include/awq_hip.h):
// the second half of scale_method="awq".  For every group of W' = RN_D(W diag(s)) the range
// [mn, mx] is shrunk by alpha_i = (n_grid - i) / n_grid, i = 0 .. n_candidates-1
// (awq_quantize_search's candidates), each candidate is scored with the scale search's own
// per-element loss x_sq[k] (RN_f32(dq / s[k]) - w)^2 (awq_act_search_losses), and the packed
// outputs are RTN of W' with the winner's range.  No reference counterpart (the reference
// stores scale_method and never reads it, awq.py:66).
//
// Two kernels with the same bits:
//   * streaming (group_size 32 / 64 / 128 / 256 dividing K, 16-B aligned w / col_scale / x_sq):
//     one wave per 2048-element tile, taken as four 512-element quarters in turn — per
//     quarter a lane holds ONE 8-element chunk with its columns' s, 1/s and x_sq in registers
//     (24 floats) across the candidate loop, so the whole search runs from registers with no
//     scratch and no LDS traffic; a group's L = group_size / 8 lanes all evaluate its
//     candidate parameters (no broadcast), the range and loss reductions are DPP steps;
//   * fallback (any power-of-two group_size in [8, 512], element-aligned pointers): one wave
//     per qzeros word, its groups in turn, lane c = chunk c of the group, wave-wide
//     reductions.  Correct, not fast.
// Both go through clip_group below: the per-op arithmetic is the streaming quantizer's
// (awq_quant.h: group_range, params_from_range, F::quot, quant8_fast / quant8_special), the
// candidate rule is awq_fast.hip search_range's, the loss chain is awq_actsearch.hip's.
#include "awq_quant.h"

namespace awq {
namespace {

// ---- group reductions -------------------------------------------------------------------
// Streaming kernel: the L consecutive lanes of a group (DPP inside 16-lane rows, one
// v_permlane16_swap for L = 32).  The sum adds own + partner at every level: the pairwise
// tree over adjacent chunks that awq_quantize_search defines (awq_lanes.h).
template <int L>
struct RedGroup {
    __device__ static int imax(int v) { return grp_max<L>(v); }
    __device__ static uint32_t umax(uint32_t v) { return grp_max<L>(v); }
    __device__ static float sum(float v) { return grp_sum<L>(v); }
};
// Fallback kernel: the whole wave is one group (xor butterfly = the same tree over 64 chunk
// slots; lanes past the group's chunks add +0 and repeat the last chunk for the maxima).
struct RedWave {
    __device__ static int imax(int v) { return wave_max_up(v); }
    __device__ static uint32_t umax(uint32_t v) { return wave_max_up(v); }
    __device__ static float sum(float v) { return wave_sum(v); }
};

// One candidate's loss over this lane's chunk: q (awq.py:245-248) of w', dq = fp16(fp16(q - z) *
// fp16(scale)) (awq.py:459-539), d = RN_f32(dq / s[k]) - w, c = x_sq[k] (d d), summed in element
// order from +0.  MQ: the quotient through the reciprocals, else the IEEE division.
template <typename F, int BITS, bool SYM, bool MQ>
__device__ __forceinline__ float chunk_loss(const Chunk<F::NW>& v, const float (&w)[8], const float (&cs)[8],
                                            const float (&rs)[8], const float (&xs)[8], const GroupParams& p) {
    constexpr float QMIN = SYM ? -(float)(1 << (BITS - 1)) : 0.0f;
    constexpr float QMAX = SYM ? (float)((1 << (BITS - 1)) - 1) : (float)((1 << BITS) - 1);
    const float zf = F::as_fmt(p.z);
    const float sh = F::dq_scale(p.s);
    const bool special = !F::fast(p.r);   // scale 0 / inf / NaN: exact division, NaN-propagating clamp
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float x = F::elem(v, i);
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
        const float dq = (float)(_Float16)opaque((q - zf) * sh);
        const float wh = MQ ? mquot(dq, cs[i], rs[i]) : dq / cs[i];
        const float d = wh - w[i];
        acc = acc + xs[i] * (d * d);
    }
    return acc;
}

struct ClipResult {
    GroupParams p;     // the winner's parameters
    bool gnan;         // the group holds a NaN
    int best;          // winning candidate
    float loss0, lossw;
    u2v word;          // this lane's 8 packed fields
};

// The whole definition for one group, seen from one lane: w = the lane's 8 original weights,
// cs / rs / xs its columns' scale, reciprocal (have_rs) and statistic; `active` = the lane's
// chunk belongs to the group (fallback kernel: lanes past the group add +0).
template <typename F, int BITS, bool SYM, typename Red>
__device__ __forceinline__ ClipResult clip_group(const float (&w)[8], const float (&cs)[8], const float (&rs)[8],
                                                 bool have_rs, const float (&xs)[8], bool active, int n_grid,
                                                 int n_cand) {
    // w' = RN_D(w s[k]) (awq_apply_input_scale)
    float y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = F::rn(w[i] * cs[i]);
    const Chunk<F::NW> v = make_chunk<F>(y);
    // the group's [mn, mx] from the raw bits, as the streaming quantizer (awq.py:192-199)
    int sm;
    uint32_t um;
    F::lane_max(v, sm, um);
    const int smax = Red::imax(sm);
    const uint32_t umax = Red::umax(um);
    const uint32_t umin = F::kOnes - Red::umax(F::lane_cmax(v));
    float gmn, gmx;
    bool gnan;
    group_range<F, SYM>(smax, umax, umin, gmn, gmx, gnan);
    // candidates: first strict minimum wins, a NaN loss never does
    float best = __builtin_inff(), loss0 = 0.0f;
    int bi = 0;
    for (int i = 0; i < n_cand; ++i) {
        const float al = clip_alpha(n_grid, i);
        const GroupParams cp = params_from_range<F, BITS, SYM>(clip_shrink<F>(gmn, al), clip_shrink<F>(gmx, al));
        float e;
        if (have_rs) {
            e = chunk_loss<F, BITS, SYM, true>(v, w, cs, rs, xs, cp);
            // a NaN loss (an out-of-range reciprocal is NaN; so is a NaN statistic): the wave
            // redoes the candidate with IEEE divisions — the same bits wherever the quotient is exact
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(e != e) != 0, 0))
                e = chunk_loss<F, BITS, SYM, false>(v, w, cs, rs, xs, cp);
        } else {
            e = chunk_loss<F, BITS, SYM, false>(v, w, cs, rs, xs, cp);
        }
        e = Red::sum(active ? e : 0.0f);
        if (i == 0) loss0 = e;
        if (e < best) {
            best = e;
            bi = i;
        }
    }
    if (!gnan && bi != 0) {
        const float al = clip_alpha(n_grid, bi);
        gmn = clip_shrink<F>(gmn, al);
        gmx = clip_shrink<F>(gmx, al);
    }
    ClipResult o;
    o.gnan = gnan;
    o.best = gnan ? 0 : bi;
    o.loss0 = loss0;
    o.lossw = o.best == 0 ? loss0 : best;
    o.p = params_from_range<F, BITS, SYM>(gmn, gmx);
    // RTN of w' with the winner's range (awq_fast.hip compute_tile step 4)
    const float zj = SYM ? 0.0f : o.p.z;
    u2v word = quant8_fast<F, BITS, SYM, false>(v, o.p.r, zj, o.p.s);
    if (__builtin_expect(!F::fast(o.p.r), 0)) {
        uint32_t nib[8];
        int32_t qs[8];
        quant8_special<F, BITS, SYM>(v, zj, o.p.s, nib, qs);
        if (BITS == 4) {
            uint32_t acc = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) acc |= nib[i] << (4 * i);
            word.x = acc;
        } else {
            word.x = nib[0] | (nib[1] << 8) | (nib[2] << 16) | (nib[3] << 24);
            word.y = nib[4] | (nib[5] << 8) | (nib[6] << 16) | (nib[7] << 24);
        }
    }
    o.word = word;
    return o;
}

struct ClipArgs {
    const void* w;
    const float* cs;
    const float* rs;       // or nullptr
    const float* xs;
    int32_t* qweight;
    int32_t* qzeros;
    uint16_t* scales;
    int32_t* best_idx;
    float* loss;           // [2, loss_stride] or nullptr
    int64_t loss_stride;
    int64_t rows, K;
    int n_grid, n_cand;
    uint32_t nan_code;
};

// per-group scalars, written by one lane of the group (fg = flat group index r G + g)
__device__ __forceinline__ void store_group(const ClipArgs& a, int64_t fg, const ClipResult& o) {
    if (a.scales) a.scales[fg] = f16_bits(o.p.s, o.gnan, a.nan_code);
    if (a.best_idx) a.best_idx[fg] = o.best;
    if (a.loss) {
        a.loss[fg] = o.loss0;
        a.loss[a.loss_stride + fg] = o.lossw;
    }
}

// ---- streaming kernel ---------------------------------------------------------------------
// Tile t = flat elements [2048 t, 2048 t + 2048) = S = 2048 / GS whole groups (K % GS == 0), in
// four quarters of 512: lane l of quarter j holds elements 512 j + 8 l .. + 7 (one 16-B load,
// two for fp32), its packed word(s) go out directly (the 64 lanes' words are consecutive).
// The tile's zero-point fields meet in LDS; a qzeros word whose groups all lie in the tile is
// stored, a word shared with a neighbouring tile (only when G % (32 / BITS) != 0; the launcher
// has zeroed qzeros then) is OR-ed in atomically.
template <typename F, int BITS, bool SYM, int GS>
__global__ __launch_bounds__(64) void clip_stream_kernel(ClipArgs a) {
    constexpr int L = GS / 8;                 // lanes per group
    constexpr uint32_t S = kTileElems / GS;   // groups per tile
    constexpr uint32_t C = 32u / BITS;        // groups per qzeros word
    __shared__ uint32_t zf[S];
    const int lane = threadIdx.x;
    const int64_t total = a.rows * a.K;
    const int64_t e0 = (int64_t)blockIdx.x * kTileElems;
    const uint32_t valid = (uint32_t)min((int64_t)kTileElems, total - e0);
    const uint32_t G = (uint32_t)(a.K / GS);
    const int64_t g0 = e0 / GS;               // first flat group of the tile
    const uint32_t ng = valid / GS;
    const uint32_t k32 = (uint32_t)a.K;
    const uint32_t col0 = (uint32_t)(e0 % a.K);
    const __amdgpu_buffer_rsrc_t rw = rsrc((const char*)a.w + e0 * F::kBytes, valid * (uint32_t)F::kBytes);
    const bool have_rs = a.rs != nullptr;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        const uint32_t el = 512u * j + 8u * lane;          // element of the tile
        if (512u * j >= valid) break;                       // wave-uniform: quarter past the tensor
        const bool in = el < valid;                         // whole groups are in or out (valid % GS == 0)
        Chunk<F::NW> raw;
#pragma unroll
        for (int h = 0; h < F::NW; ++h)
            raw.w[h] = __builtin_amdgcn_raw_buffer_load_b128(rw, el * (uint32_t)F::kBytes + 16u * h, 0, AWQ_LOAD_AUX);
        // the chunk's columns (a chunk never straddles rows: K % 8 == 0); lanes past the tensor
        // read some valid column and store nothing
        const uint32_t col = (col0 + el) % k32;
        const float4 s0 = *(const float4*)(a.cs + col), s1 = *(const float4*)(a.cs + col + 4);
        const float4 x0 = *(const float4*)(a.xs + col), x1 = *(const float4*)(a.xs + col + 4);
        const float cs[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        const float xs[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        float rs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (have_rs) {
            const float4 r0 = *(const float4*)(a.rs + col), r1 = *(const float4*)(a.rs + col + 4);
            rs[0] = r0.x; rs[1] = r0.y; rs[2] = r0.z; rs[3] = r0.w;
            rs[4] = r1.x; rs[5] = r1.y; rs[6] = r1.z; rs[7] = r1.w;
        }
        float w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = F::elem(raw, i);
        const ClipResult o = clip_group<F, BITS, SYM, RedGroup<L>>(w, cs, rs, have_rs, xs, true, a.n_grid, a.n_cand);
        if (in && a.qweight) {
            int32_t* qw = a.qweight + (e0 + el) / 8 * (BITS / 4);
            qw[0] = (int32_t)o.word.x;
            if (BITS == 8) qw[1] = (int32_t)o.word.y;
        }
        const uint32_t slot = el / GS;
        if (in && lane % L == 0) {
            store_group(a, g0 + slot, o);
            zf[slot] = zero_field<BITS, SYM>(o.p.z);
        }
    }
    if (!a.qzeros) return;
    __syncthreads();
    // qzeros words touched by the tile: consecutive (every word holds a group of the tile)
    const uint32_t WPR = (G + C - 1) / C;
    const int64_t r0 = g0 / G, rl = (g0 + ng - 1) / G;
    const int64_t W0 = r0 * WPR + (uint32_t)(g0 - r0 * G) / C;
    const int64_t W1 = rl * WPR + (uint32_t)(g0 + ng - 1 - rl * G) / C;
    const int64_t W = W0 + lane;
    if (W > W1) return;
    const int64_t r = W / WPR;
    const uint32_t gi0 = (uint32_t)(W - r * WPR) * C;
    const uint32_t cnt = min(C, G - gi0);
    const int64_t f0 = r * G + gi0;           // the word's first flat group
    uint32_t val = 0;
    bool whole = true;
    for (uint32_t t = 0; t < cnt; ++t) {
        const int64_t rel = f0 + t - g0;
        if (rel >= 0 && rel < (int64_t)ng) val |= zf[rel] << (BITS * t);
        else whole = false;
    }
    if (whole) a.qzeros[W] = (int32_t)val;
    else atomicOr((unsigned int*)a.qzeros + W, val);
}

// ---- fallback kernel ------------------------------------------------------------------------
// One wave per qzeros word (C = 32 / BITS groups of one row, fewer at the row end), the groups in
// turn; lane c < gs / 8 holds chunk c, loaded element by element (pointers only element-aligned).
template <typename F, int BITS, bool SYM>
__global__ __launch_bounds__(64) void clip_group_kernel(ClipArgs a, int gs) {
    constexpr uint32_t C = 32u / BITS;
    typedef typename std::conditional<F::NW == 2, uint32_t, uint16_t>::type E;
    const int lane = threadIdx.x;
    const int64_t G = a.K / gs;
    const int64_t WPR = (G + C - 1) / C;
    const int64_t W = blockIdx.x;
    const int64_t r = W / WPR;
    const int64_t gi0 = (W - r * WPR) * C;
    const int cnt = (int)min((int64_t)C, G - gi0);
    const int nch = gs / 8;
    const bool active = lane < nch;
    const int ch = active ? lane : nch - 1;   // lanes past the group repeat its last chunk
    const bool have_rs = a.rs != nullptr;
    uint32_t zword = 0;
    for (int t = 0; t < cnt; ++t) {
        const int64_t g = gi0 + t;
        const int64_t k0 = g * gs + 8 * ch;
        const E* src = (const E*)a.w + r * a.K + k0;
        float w[8], cs[8], xs[8], rs[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            w[i] = F::dec(src[i]);
            cs[i] = a.cs[k0 + i];
            xs[i] = a.xs[k0 + i];
            rs[i] = have_rs ? a.rs[k0 + i] : 0.0f;
        }
        const ClipResult o = clip_group<F, BITS, SYM, RedWave>(w, cs, rs, have_rs, xs, active, a.n_grid, a.n_cand);
        if (active && a.qweight) {
            int32_t* qw = a.qweight + (r * a.K + k0) / 8 * (BITS / 4);
            qw[0] = (int32_t)o.word.x;
            if (BITS == 8) qw[1] = (int32_t)o.word.y;
        }
        if (lane == 0) store_group(a, r * G + g, o);
        zword |= zero_field<BITS, SYM>(o.p.z) << (BITS * t);
    }
    if (lane == 0 && a.qzeros) a.qzeros[W] = (int32_t)zword;
}

template <typename F>
void launch_clip(bool stream_ok, int gs, int bits, int sym, unsigned grid, hipStream_t st, const ClipArgs& a) {
#define AWQ_CLIP_GS(B, S)                                                                                    \
    switch (gs) {                                                                                            \
    case 32: hipLaunchKernelGGL((clip_stream_kernel<F, B, S, 32>), dim3(grid), dim3(64), 0, st, a); break;   \
    case 64: hipLaunchKernelGGL((clip_stream_kernel<F, B, S, 64>), dim3(grid), dim3(64), 0, st, a); break;   \
    case 128: hipLaunchKernelGGL((clip_stream_kernel<F, B, S, 128>), dim3(grid), dim3(64), 0, st, a); break; \
    default: hipLaunchKernelGGL((clip_stream_kernel<F, B, S, 256>), dim3(grid), dim3(64), 0, st, a); break;  \
    }
#define AWQ_CLIP(B, S)                                                                                       \
    do {                                                                                                     \
        if (stream_ok) { AWQ_CLIP_GS(B, S) }                                                                 \
        else hipLaunchKernelGGL((clip_group_kernel<F, B, S>), dim3(grid), dim3(64), 0, st, a, gs);           \
    } while (0)
    switch ((bits == 8 ? 2 : 0) + (sym ? 1 : 0)) {
    case 0: AWQ_CLIP(4, false); break;
    case 1: AWQ_CLIP(4, true); break;
    case 2: AWQ_CLIP(8, false); break;
    default: AWQ_CLIP(8, true); break;
    }
#undef AWQ_CLIP
#undef AWQ_CLIP_GS
}

}  // namespace
}  // namespace awq

using namespace awq;

extern "C" int awq_quantize_clip_scaled(const void* w, int dtype, int64_t rows, int64_t K, int32_t group_size32,
                                        int bits, int symmetric, const float* col_scale, const float* col_rscale,
                                        const float* x_sq, int n_grid, int n_candidates, int32_t* qweight,
                                        int32_t* qzeros, uint16_t* scales, int32_t* best_idx, float* group_loss,
                                        int64_t loss_stride, void* stream) {
    set_error(AWQ_OK, "");
    const long long gs = group_size32, R = rows, KK = K;   // (long long: the messages' %lld)
    if (bits != 4 && bits != 8) return fail(AWQ_EINVAL, "Unsupported bit width: %d. Supported: 4, 8.", bits);
    if (gs <= 0) return fail(AWQ_EINVAL, "Group size must be a positive integer: %lld", gs);
    if (rows < 0 || K < 0) return fail(AWQ_EINVAL, "negative shape (%lld, %lld)", R, KK);
    if (dtype == AWQ_DTYPE_F64) return fail(AWQ_EUNSUPPORTED, "awq_quantize_clip_scaled: fp64 weights are not supported");
    if (dtype < AWQ_DTYPE_BF16 || dtype > AWQ_DTYPE_F32)
        return fail(AWQ_EINVAL, "awq_quantize_clip_scaled: dtype must be bf16, fp16 or fp32 (got code %d)", dtype);
    if (n_grid < 1 || n_candidates < 1 || n_candidates > n_grid)
        return fail(AWQ_EINVAL, "clip search needs 1 <= n_candidates (%d) <= n_grid (%d)", n_candidates, n_grid);
    if (!qweight && !qzeros && !scales && !best_idx && !group_loss) return fail(AWQ_EINVAL, "no output requested");
    if (rows == 0 || K == 0) return AWQ_OK;
    if (!w || !col_scale || !x_sq) return fail(AWQ_EINVAL, "null input");
    if (gs > 512)
        return fail(AWQ_EUNSUPPORTED, "awq_quantize_clip_scaled: group_size %lld > 512 is not supported", gs);
    if (gs < 8 || (gs & (gs - 1)) != 0 || K % gs != 0)
        return fail(AWQ_EUNSUPPORTED,
                    "awq_quantize_clip_scaled: group_size %lld must be a power of two in [8, 512] dividing K = %lld", gs, KK);
    const long long G = K / gs;
    if (G > (int64_t)0x7FFFFFFF / rows || K > ((int64_t)1 << 40) / rows)
        return fail(AWQ_EUNSUPPORTED, "awq_quantize_clip_scaled: %lld x %lld groups exceed the kernels' range", R, G);
    if (group_loss && loss_stride < rows * G)
        return fail(AWQ_EINVAL, "group_loss needs loss_stride (%lld) >= rows * G (%lld)", (long long)loss_stride, R * G);
    const size_t esz = dtype == AWQ_DTYPE_F32 ? 4 : 2;
    if (!aligned(w, esz) || !aligned(col_scale, 4) || !aligned(col_rscale, 4) || !aligned(x_sq, 4) ||
        !aligned(qweight, 4) || !aligned(qzeros, 4) || !aligned(scales, 2) || !aligned(best_idx, 4) ||
        !aligned(group_loss, 4))
        return fail(AWQ_EINVAL, "awq_quantize_clip_scaled: a pointer is not aligned to its element size");
    hipStream_t st = (hipStream_t)stream;
    const int64_t C = 32 / bits, WPR = (G + C - 1) / C;
    const int64_t tiles = (rows * K + kTileElems - 1) / kTileElems;
    const bool stream_ok = fast_group_size(gs) && aligned(w, 16) && aligned(col_scale, 16) && aligned(x_sq, 16) &&
                           (!col_rscale || aligned(col_rscale, 16));
    const int64_t blocks = stream_ok ? tiles : rows * WPR;
    if (blocks > (int64_t)0x7FFFFFFF)
        return fail(AWQ_EUNSUPPORTED, "awq_quantize_clip_scaled: %lld x %lld is beyond one launch's grid", R, KK);
    ClipArgs a;
    a.w = w; a.cs = col_scale; a.rs = col_rscale; a.xs = x_sq;
    a.qweight = qweight; a.qzeros = qzeros; a.scales = scales; a.best_idx = best_idx;
    a.loss = group_loss; a.loss_stride = loss_stride;
    a.rows = rows; a.K = K; a.n_grid = n_grid; a.n_cand = n_candidates;
    a.nan_code = nan_scale_code(dtype, symmetric, false);
    hipError_t e = hipSuccess;
    // qzeros words shared by two tiles are OR-ed into zeroed memory (streaming kernel)
    if (stream_ok && qzeros && G % C != 0) e = hipMemsetAsync(qzeros, 0, (size_t)(rows * WPR) * 4, st);
    if (e == hipSuccess) {
        if (dtype == AWQ_DTYPE_BF16) launch_clip<FmtBF16>(stream_ok, (int)gs, bits, symmetric, (unsigned)blocks, st, a);
        else if (dtype == AWQ_DTYPE_F16) launch_clip<FmtF16>(stream_ok, (int)gs, bits, symmetric, (unsigned)blocks, st, a);
        else launch_clip<FmtF32>(stream_ok, (int)gs, bits, symmetric, (unsigned)blocks, st, a);
        e = hipPeekAtLastError();
    }
    return hip_status(e, "awq clip kernels");
}
