// awq_lanes.h — the one home of the cross-lane reductions every kernel file uses (awq_fast,
// awq_rowgroup, awq_qerror, awq_actclip, awq_actsearch through awq_quant.h; awq_generic through
// awq_refmath.h).  Header-only, anonymous namespace: each including file gets its own copies.
//
// The tree.  A reduction over the lpg consecutive lanes of a group (lpg a power of two, 2..64)
// is the xor butterfly with growing offsets: lane l combines with lane l ^ 1, then l ^ 2, ...,
// l ^ (lpg / 2), so every lane of the group ends with the same value.  Inside a 16-lane row the
// steps are DPP moves (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror:
// after the earlier steps the mirrors pair exactly the lanes the xor pairs), across rows
// v_permlane16_swap / v_permlane32_swap (gfx950).  For a sum that is the pairwise tree over
// adjacent lanes, adjacent pairs first, own + partner at every level (fp addition commutes):
// the canonical summation order include/awq_hip.h defines (awq_quantize_search, awq_act_*) and
// oracle/awq_oracle.c restates.  Changing a step here changes the bits of every kernel at once;
// or / min / max are order-free.
//
// Recorded counter figures: bench.py marks profiles/round6/pmc_*.json stale from a hash over
// awq_fast.hip / awq_quant.h / awq_internal.h (streaming kernel) and awq_actsearch.hip /
// awq_refmath.h / awq_internal.h (loss kernels).  This file is in neither list, although both
// measured kernels take their reductions (and the loss kernels their inline-asm DPP min / max)
// from here: an edit to this file does NOT mark those records stale.  After one, compare the
// assembly (scripts/isa_diff.py REV) and, if a measured kernel changed, re-record the figures.
#ifndef AWQ_LANES_H
#define AWQ_LANES_H
#include "awq_internal.h"

namespace awq {
namespace {

// one butterfly step's operand: the DPP-permuted copy of a 32-bit v (full row / bank masks,
// every source lane valid) — LLVM folds the move into the op that uses it (v_add_f32_dpp,
// v_max_i32_dpp, ...: one instruction)
template <int CTRL, typename T>
__device__ __forceinline__ T dpp_mov(T v) {
    return __builtin_bit_cast(T, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// one step of a sum: own + partner (a function of its own, not `v + dpp_mov(v)` written out in
// the tree: the operand order of the integer adds the compiler emits depends on it)
template <int CTRL, typename T>
__device__ __forceinline__ T dpp_add(T v) {
    return v + dpp_mov<CTRL>(v);
}
// the two 16-lane rows (swap16) or 32-lane halves (swap32) of a pair, swapped: lane l gets {its
// pair's first half, its pair's second half} whichever half it is in, so combining a and b
// symmetrically (+, |, min, max) gives every lane f(own, partner) exactly
template <typename T>
__device__ __forceinline__ void swap16(T v, T& a, T& b) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto p = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    a = __builtin_bit_cast(T, (unsigned)p[0]);
    b = __builtin_bit_cast(T, (unsigned)p[1]);
}
template <typename T>
__device__ __forceinline__ void swap32(T v, T& a, T& b) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto p = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    a = __builtin_bit_cast(T, (unsigned)p[0]);
    b = __builtin_bit_cast(T, (unsigned)p[1]);
}

// ---- group reductions.  Lanes per group: the template constant L (grp_sum<L>(v): the steps are
// chosen at compile time) or the wave-uniform run-time lpg (grp_sum(v, lpg)); one body each ----
template <int L, typename T>   // L = 0: n lanes at run time
__device__ __forceinline__ T grp_sum_steps(T v, int lpg) {
    const int n = L ? L : lpg;
    if (n >= 2) v = dpp_add<0xB1>(v);     // quad_perm [1,0,3,2]
    if (n >= 4) v = dpp_add<0x4E>(v);     // quad_perm [2,3,0,1]
    if (n >= 8) v = dpp_add<0x141>(v);    // row_half_mirror
    if (n >= 16) v = dpp_add<0x140>(v);   // row_mirror
    T a, b;
    if (n >= 32) { swap16(v, a, b); v = a + b; }   // (row 2k) + (row 2k+1) on both rows
    if (n >= 64) { swap32(v, a, b); v = a + b; }
    return v;
}
template <int L, typename T>
__device__ __forceinline__ T grp_max_steps(T v, int lpg) {
    const int n = L ? L : lpg;
    if (n >= 2) v = max(v, dpp_mov<0xB1>(v));
    if (n >= 4) v = max(v, dpp_mov<0x4E>(v));
    if (n >= 8) v = max(v, dpp_mov<0x141>(v));
    if (n >= 16) v = max(v, dpp_mov<0x140>(v));
    T a, b;
    if (n >= 32) { swap16(v, a, b); v = max(a, b); }
    if (n >= 64) { swap32(v, a, b); v = max(a, b); }
    return v;
}
template <int L, typename T>   // T = float or int
__device__ __forceinline__ T grp_sum(T v) {
    static_assert(L >= 2 && L <= 64 && (L & (L - 1)) == 0, "lanes per group");
    return grp_sum_steps<L>(v, L);
}
template <typename T>
__device__ __forceinline__ T grp_sum(T v, int lpg) { return grp_sum_steps<0>(v, lpg); }
template <int L, typename T>   // T = int (signed max) or uint32_t (unsigned max)
__device__ __forceinline__ T grp_max(T v) {
    static_assert(L >= 2 && L <= 64 && (L & (L - 1)) == 0, "lanes per group");
    return grp_max_steps<L>(v, L);
}
template <typename T>
__device__ __forceinline__ T grp_max(T v, int lpg) { return grp_max_steps<0>(v, lpg); }
__device__ __forceinline__ int grp_or(int v, int lpg) {
    if (lpg >= 2) v |= dpp_mov<0xB1>(v);
    if (lpg >= 4) v |= dpp_mov<0x4E>(v);
    if (lpg >= 8) v |= dpp_mov<0x141>(v);
    if (lpg >= 16) v |= dpp_mov<0x140>(v);
    int a, b;
    if (lpg >= 32) { swap16(v, a, b); v = a | b; }
    if (lpg >= 64) { swap32(v, a, b); v = a | b; }
    return v;
}

// ---- float min / max (the activation-aware search's group ranges) ----
// min(a, b) / max(a, b) as v_med3 against -inf / +inf: no NaN-quieting of the DPP-moved
// operand (fminf / fmaxf need it in IEEE mode); NaN is tracked on the side, so no operand is
// NaN whenever the result is used
__device__ __forceinline__ float min2(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, -__builtin_inff()); }
__device__ __forceinline__ float max2(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, __builtin_inff()); }

template <bool ROW32>
__device__ __forceinline__ void minmax_cross(float& mn, float& mx, int& nan) {
    float a, b;
    int p, q;
    if (ROW32) swap32(mn, a, b); else swap16(mn, a, b);
    mn = min2(a, b);
    if (ROW32) swap32(mx, a, b); else swap16(mx, a, b);
    mx = max2(a, b);
    if (ROW32) swap32(nan, p, q); else swap16(nan, p, q);
    nan = p | q;
}
// min, max and the NaN flag together
__device__ __forceinline__ void grp_minmax(float& mn, float& mx, int& nan, int lpg) {
    if (lpg >= 2) { mn = min2(mn, dpp_mov<0xB1>(mn)); mx = max2(mx, dpp_mov<0xB1>(mx)); nan |= dpp_mov<0xB1>(nan); }
    if (lpg >= 4) { mn = min2(mn, dpp_mov<0x4E>(mn)); mx = max2(mx, dpp_mov<0x4E>(mx)); nan |= dpp_mov<0x4E>(nan); }
    if (lpg >= 8) { mn = min2(mn, dpp_mov<0x141>(mn)); mx = max2(mx, dpp_mov<0x141>(mx)); nan |= dpp_mov<0x141>(nan); }
    if (lpg >= 16) { mn = min2(mn, dpp_mov<0x140>(mn)); mx = max2(mx, dpp_mov<0x140>(mx)); nan |= dpp_mov<0x140>(nan); }
    if (lpg >= 32) minmax_cross<false>(mn, mx, nan);
    if (lpg >= 64) minmax_cross<true>(mn, mx, nan);
}

// v_min_f32 / v_max_f32 with the partner lane's operand through DPP, one instruction per step
// (the compiler turns min2 / max2 into v_min / v_max behind a canonicalising v_max x, x and a
// separate v_mov_dpp: three).  The s_nop covers the VALU-write -> DPP-read wait states (the
// operand may have been written by the instruction just before).  No NaN reaches these (the
// weights' NaN flag is tracked on the side), and the sign of a zero extreme cannot change the
// scale or zero point.
#define AWQ_DPP_MINMAX(NAME, OP, CTRL)                                                                   \
    __device__ __forceinline__ float NAME(float v) {                                                    \
        float r;                                                                                        \
        asm("s_nop 1\n\t" OP "_dpp %0, %1, %1 " CTRL " row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(r) : "v"(v)); \
        return r;                                                                                       \
    }
AWQ_DPP_MINMAX(min_xor1, "v_min_f32", "quad_perm:[1,0,3,2]")
AWQ_DPP_MINMAX(max_xor1, "v_max_f32", "quad_perm:[1,0,3,2]")
AWQ_DPP_MINMAX(min_xor2, "v_min_f32", "quad_perm:[2,3,0,1]")
AWQ_DPP_MINMAX(max_xor2, "v_max_f32", "quad_perm:[2,3,0,1]")
AWQ_DPP_MINMAX(min_hmir, "v_min_f32", "row_half_mirror")
AWQ_DPP_MINMAX(max_hmir, "v_max_f32", "row_half_mirror")
AWQ_DPP_MINMAX(min_mir, "v_min_f32", "row_mirror")
AWQ_DPP_MINMAX(max_mir, "v_max_f32", "row_mirror")
#undef AWQ_DPP_MINMAX

// the group min / max alone (the weights' NaN flag is reduced once per item: grp_or)
__device__ __forceinline__ void grp_minmax_nn(float& mn, float& mx, int lpg) {
    if (lpg >= 2) { mn = min_xor1(mn); mx = max_xor1(mx); }
    if (lpg >= 4) { mn = min_xor2(mn); mx = max_xor2(mx); }
    if (lpg >= 8) { mn = min_hmir(mn); mx = max_hmir(mx); }
    if (lpg >= 16) { mn = min_mir(mn); mx = max_mir(mx); }
    // the compiler's hazard tracking does not see into the asm: wait states before the cross-row
    // swaps below read its results
    if (lpg >= 32) asm volatile("s_nop 1" : "+v"(mn), "+v"(mx));
    int dummy = 0;
    if (lpg >= 32) minmax_cross<false>(mn, mx, dummy);
    if (lpg >= 64) minmax_cross<true>(mn, mx, dummy);
}

// ---- whole-wave butterflies (__shfl_xor over all 64 lanes; T = float, double, int, uint32_t) ----
// the sum: growing offsets = the canonical tree over 64 slots (the group reductions above are
// its first levels; oracle_quantize_search restates it)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}
// min / max / or are order-free: the same bits from either direction, but not the same code, so
// both stay.  Shrinking offsets with a compare-and-select (a NaN never wins): awq_generic.hip
template <typename C> __device__ __forceinline__ C wave_min(C v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { C t = __shfl_xor(v, o, 64); v = t < v ? t : v; }
    return v;
}
template <typename C> __device__ __forceinline__ C wave_max(C v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { C t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    return v;
}
__device__ __forceinline__ int wave_or(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}
// growing offsets with max() on raw bit patterns (int / uint32_t): awq_actclip.hip's fallback
template <typename T>
__device__ __forceinline__ T wave_max_up(T v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = max(v, (T)__shfl_xor((int)v, o, 64));
    return v;
}

}  // namespace
}  // namespace awq
#endif  // AWQ_LANES_H
