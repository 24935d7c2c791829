// awq_gemm_layout.h — what the AutoAWQ "GEMM" layout kernels share (awq_export.hip, its inverse
// awq_import.hip): the interleave AWQ_ORDER, the tile geometry and the in-register 8 x 8 nibble
// transpose.
#pragma once

#include "awq_internal.h"

namespace awq {

#ifndef AWQ_EXPORT_NT_MIN
// qweight outputs of at least this many bytes are stored nontemporal (past the caches:
// larger than half the 256 MB MALL they only evict; smaller ones gain from write-back)
#define AWQ_EXPORT_NT_MIN (128ll << 20)
#endif
// nibble i of a GEMM-layout word c holds column 8c + kAwqOrder[i]
constexpr int kAwqOrder[8] = {0, 2, 4, 6, 1, 3, 5, 7};
constexpr int kT2 = 256;                 // qweight tile edge in nibbles (n and k)
constexpr int kGN = 64, kGG = 32;        // scales / qzeros tile: 64 (n) x 32 (g)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ void swapn(uint32_t& x, uint32_t& y, int sh, uint32_t mask) {
    const uint32_t t = ((x >> sh) ^ y) & mask;
    x ^= t << sh;
    y ^= t;
}
// rows a[0..7] (8 nibbles each) -> b[j] = nibble j of every row, row AWQ_ORDER[i] at nibble i
// (the rows taken in AWQ_ORDER by register renaming, then three rounds of masked swaps)
static __device__ __forceinline__ void nibble_transpose8(const uint32_t (&a)[8], uint32_t (&b)[8]) {
    b[0] = a[0]; b[1] = a[2]; b[2] = a[4]; b[3] = a[6];
    b[4] = a[1]; b[5] = a[3]; b[6] = a[5]; b[7] = a[7];
#pragma unroll
    for (int i = 0; i < 4; ++i) swapn(b[i], b[i + 4], 16, 0x0000FFFFu);
#pragma unroll
    for (int i = 0; i < 8; i += 4) {
        swapn(b[i], b[i + 2], 8, 0x00FF00FFu);
        swapn(b[i + 1], b[i + 3], 8, 0x00FF00FFu);
    }
#pragma unroll
    for (int i = 0; i < 8; i += 2) swapn(b[i], b[i + 1], 4, 0x0F0F0F0Fu);
}
// the inverse: GEMM-layout words a[r] (nibble i = column AWQ_ORDER[i] of row r) -> b[m] = nibble
// r of every word for column m.  The same transpose between two renamings: its input taken in
// the reverse order (so it sees the rows in sequence), its outputs put back by AWQ_ORDER.
static __device__ __forceinline__ void nibble_untranspose8(const uint32_t (&a)[8], uint32_t (&b)[8]) {
    const uint32_t ap[8] = {a[0], a[4], a[1], a[5], a[2], a[6], a[3], a[7]};
    uint32_t t[8];
    nibble_transpose8(ap, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) b[kAwqOrder[j]] = t[j];
}

}  // namespace awq
