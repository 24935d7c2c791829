// awq_mxfp4.h — the MXFP4 block arithmetic two kernel files share (awq_mxfp4.hip: awq_quantize_mxfp4;
// awq_act_mxfp4.hip: awq_quantize_mxfp4_scaled, awq_act_search_losses_mxfp4): the scale rule and the
// element rounding of a block held by a quad of lanes, 8 elements each, the gather and store of a
// 2048-element segment's scale bytes, and the shape checks of the entry points.  The definitions and
// why they give the format's bits: awq_mxfp4.hip's head comment.  Header-only, anonymous namespace:
// each including file gets its own copies.
#pragma once
#include "awq_quant.h"

namespace awq {
namespace {

constexpr int kBlockElems = 32;             // elements per MXFP4 block
constexpr unsigned kQuantWaves = 256 * 32;  // the quantize grid's cap: waves (= one-wave workgroups)

// max of the 8 |x| bit patterns of a lane's chunk (sign-magnitude formats: the order of the
// magnitudes is the order of the patterns)
template <typename F>
__device__ __forceinline__ uint32_t lane_absmax(const Chunk<F::NW>& c) {
    if constexpr (F::NW == 1) {
        const uint32_t x0 = c.w[0].x & 0x7FFF7FFFu, x1 = c.w[0].y & 0x7FFF7FFFu;
        const uint32_t x2 = c.w[0].z & 0x7FFF7FFFu, x3 = c.w[0].w & 0x7FFF7FFFu;
        const us2 m = __builtin_elementwise_max(__builtin_elementwise_max(as_us2(x0), as_us2(x1)),
                                                __builtin_elementwise_max(as_us2(x2), as_us2(x3)));
        return max((uint32_t)m.x, (uint32_t)m.y);
    } else {
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) m = max(m, (uint32_t)c.w[i >> 2][i & 3] & 0x7FFFFFFFu);
        return m;
    }
}

// A lane's 8 elements at the scale 2^-X = inv: the 8 codes as one dword and, with ERR, the sum of
// (v - rounded v)^2 in element order from +0.
template <typename F, bool ERR>
__device__ __forceinline__ uint32_t quant8(const Chunk<F::NW>& c, float inv, float& err) {
    uint32_t word = 0;
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float x = F::elem(c, i);
        const float t = __builtin_fabsf(x) * inv;
        const float v = __builtin_fminf(t, 6.0f);
        const uint32_t k = max(__float_as_uint(v) >> 23, 127u);        // 127, 128, 129
        const float magic = __uint_as_float((k + 22u) << 23);
        const float r = v + magic;                                     // the one rounding
        const uint32_t code = (__float_as_uint(r) & 7u) + 2u * k - 254u;
        word |= (code | ((__float_as_uint(x) >> 28) & 8u)) << (4 * i);
        if (ERR) {
            const float d = t - (r - magic);
            s = s + d * d;
        }
    }
    err = s;
    return word;
}

// One block = one quad, every lane its 8 elements in v: the block's scale byte under RULE (255: the
// block holds a NaN or an inf) and the lane's dword of codes (0 in such a block).
template <typename F, int RULE>
__device__ __forceinline__ uint32_t mxfp4_block(const Chunk<F::NW>& v, uint32_t& word) {
    const uint32_t amax = grp_max<4, uint32_t>(lane_absmax<F>(v));
    const bool bad = amax >= (uint32_t)F::kNanS;                       // exponent all ones
    const float af = F::dec(amax);
    uint32_t e = amax == 0u ? 127u : max(__float_as_uint(af) >> 23, 2u) - 2u;
    const float inv = __uint_as_float((254u - e) << 23);               // 2^-X, e <= 252
    float s0 = 0.0f, s1 = 0.0f;
    if (RULE == AWQ_MXFP4_MSE) {
        word = quant8<F, true>(v, inv, s0);
        const uint32_t w1 = quant8<F, true>(v, inv * 0.5f, s1);
        const bool up = 4.0f * grp_sum<4>(s1) < grp_sum<4>(s0);
        word = up ? w1 : word;
        e += up ? 1u : 0u;
    } else {
        const bool up = RULE == AWQ_MXFP4_CEIL && af * inv > 6.0f;
        e += up ? 1u : 0u;
        word = quant8<F, false>(v, up ? inv * 0.5f : inv, s0);
    }
    word = bad ? 0u : word;
    return bad ? 255u : e;
}

// The 16 scale bytes of load j of a segment, gathered over each 16-lane row (byte position = the
// quad's place in the row, or-ed over the row's two mirrors) into one dword per row; lane j of a row
// keeps load j's in sd.
__device__ __forceinline__ void gather_scale_bytes(uint32_t e, int lane, int j, uint32_t& sd) {
    uint32_t sb = e << (8 * ((lane >> 2) & 3));
    sb |= dpp_mov<0x141>(sb);   // row_half_mirror: the row's quads 0 | 1 and 2 | 3
    sb |= dpp_mov<0x140>(sb);   // row_mirror: all four
    sd = (lane & 15) == j ? sb : sd;
}

// A segment's scale bytes at sp: a whole segment (te == 2048) as 16 dwords from lanes 0..3 of every
// row, a short one byte by byte from each quad's first lane (eb[j]: the lane's block of load j).
__device__ __forceinline__ void store_scale_bytes(uint8_t* sp, uint32_t te, int lane, uint32_t sd,
                                                  const uint32_t (&eb)[4]) {
    if (te == (uint32_t)kTileElems) {
        if ((lane & 15) < 4) ((uint32_t*)sp)[(lane & 15) * 4 + (lane >> 4)] = sd;
    } else if ((lane & 3) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t b = (uint32_t)(j * 16 + (lane >> 2));
            if (b < te / kBlockElems) sp[b] = (uint8_t)eb[j];
        }
    }
}

// The scale 2^(e - 127) of a byte e < 255 as fp32 (e = 0 is the subnormal 2^-127).
__device__ __forceinline__ float fp4_scale(uint32_t e) {
    return __uint_as_float(max(e << 23, 0x00400000u));
}

// what the MXFP4 entry points check alike: 0 = fine
inline int check_common(const char* what, int dtype, int64_t rows, int64_t K) {
    if (rows < 0 || K < 0) return fail(AWQ_EINVAL, "%s: negative shape (%lld, %lld)", what, (long long)rows, (long long)K);
    if (K % kBlockElems != 0)
        return fail(AWQ_EINVAL, "%s: K %% 32 must be 0, the MXFP4 block (K=%lld)", what, (long long)K);
    if (dtype != AWQ_DTYPE_BF16 && dtype != AWQ_DTYPE_F16 && dtype != AWQ_DTYPE_F32)
        return fail(AWQ_EINVAL, "%s: dtype code %d is not bf16, fp16 or fp32", what, dtype);
    if (rows > 0 && K > ((int64_t)1 << 60) / rows)
        return fail(AWQ_EUNSUPPORTED, "%s: %lld x %lld elements exceed 2^60", what, (long long)rows, (long long)K);
    return AWQ_OK;
}
inline bool mxfp4_rule_ok(int rule) {
    return rule == AWQ_MXFP4_FLOOR || rule == AWQ_MXFP4_CEIL || rule == AWQ_MXFP4_MSE;
}

}  // namespace
}  // namespace awq
