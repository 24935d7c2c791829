// awq_mxfp4_gemm.hip — the MXFP4 x MXFP4 product on CDNA4's scaled matrix instruction (include/awq_hip.h
// awq_mxfp4_gemm): out[t, n] = sum_k a[t, k] w[n, k] (+ bias[n]), both operands in the
// layout awq_quantize_mxfp4 writes (awq_mxfp4.hip's head comment).  Self-contained: the entry point, its
// validation and the kernel.
//
// The instruction.  v_mfma_scale_f32_32x32x64_f8f6f4 with both operands E2M1 (cbsz = blgp = 4) takes, per
// lane l, 32 consecutive codes of ONE row (A: row l % 32 of the 32 x 64 slab, B: column l % 32; both the k
// range 32 (l / 32) .. + 31) as four dwords, and one E8M0 byte per lane and operand as that run's scale.
// Both operands here are K-major with 32-element blocks, so a lane's operand is one MX block as it lies in
// memory — 16 B of codes and the block's scale byte: no nibble is moved, and since A and B take the same
// 16 bytes of their rows in the same order, the order of the codes inside the run does not matter to the
// sum.  The 32 x 32 result is 16 fp32 per lane: column l % 32, rows 8 (v / 4) + 4 (l / 32) + v % 4.
//
// The split.  A workgroup of four waves makes a 128 (t) x 128 (n) tile, a wave 64 x 64 of it as 2 x 2
// instruction tiles (64 accumulator registers).  K is walked in steps of 256 elements: per operand 128 rows
// x 128 B of codes and 128 x 8 scale bytes, copied global -> registers -> LDS by all 256 threads (codes:
// four 16-B loads per thread and operand, 8 consecutive threads one row's 128 B; scales: a row's 8 bytes by
// two threads, a dword each when K / 32 % 4 == 0 and the base is 4-B aligned, byte by byte otherwise).  Two
// stages of LDS (2 x 34 KiB): the loads of step s + 1 are issued before the instructions of step s and
// written to the other stage after them, one barrier per step.  In LDS the 16-B chunk c of row r sits at
// chunk c ^ (r & 7) of the row's 128 B, so the ds_read_b128 of 32 rows at one chunk column is spread over
// all banks; the lane's scale byte comes out of the row's 8 bytes, read as one 64-bit word per row and step.
//
// Edges.  Rows beyond T / N are read from the operand's last row and never stored.  Chunks beyond K are
// zero codes with the scale byte 127 (a K % 64 == 32 tail: the second half of the last instruction adds
// +0 products); 64-slabs wholly beyond K are skipped.  The grid is one-dimensional, the t tile the fast
// index: the workgroups running at one time share a W tile (L2), A (the smaller operand of a decoder
// linear's T x N x K) is re-read per n tile.
//
// The sum of one output element: acc = +0; for every 64-slab of K in increasing order one instruction,
// acc <- acc + (the slab's 64 scaled products, combined in the hardware's order); then + bias in fp32; one
// rounding into the output type.  A scale byte 255 in row t of A or row n of W: the epilogue writes NaN
// whatever the instruction made of the byte (a per-row flag gathered while the scale bytes are read).
#include "awq_mxfp4.h"

namespace awq {
namespace {

typedef int i8v __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int kTile = 128;                          // rows of either operand per workgroup
constexpr int kStepK = 256;                         // elements of K per step
constexpr int kRowBytes = kStepK / 2;               // 128 B of codes per row and step
constexpr int kCodeBytes = kTile * kRowBytes;       // 16 KiB per operand and stage
constexpr int kScaleBytes = kTile * 8;              // 1 KiB per operand and stage
constexpr int kStageBytes = 2 * (kCodeBytes + kScaleBytes);

// a step of one operand in flight: a thread's four 16-B code chunks and its four scale bytes
struct Fetch {
    u4 c[4];
    uint32_t s;
};

__device__ __forceinline__ Fetch fetch(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                                       int64_t rows, int64_t row0, int64_t K, int64_t k0, bool scale_dwords,
                                       int tid) {
    Fetch f;
    const int64_t kbytes = K / 2, KB = K / kBlockElems;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int chunk = tid + 256 * j;
        const int64_t row = min(row0 + (chunk >> 3), rows - 1);
        const int64_t off = k0 / 2 + (chunk & 7) * 16;
        f.c[j] = off < kbytes ? *(const u4*)(codes + row * kbytes + off) : (u4){0u, 0u, 0u, 0u};
    }
    const int64_t row = min(row0 + (tid >> 1), rows - 1);
    const int64_t kb = k0 / kBlockElems + (tid & 1) * 4;
    const uint8_t* sp = scales + row * KB + kb;
    if (scale_dwords) {
        f.s = kb < KB ? *(const uint32_t*)sp : 0x7F7F7F7Fu;
    } else {
        f.s = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) f.s |= (kb + b < KB ? (uint32_t)sp[b] : 127u) << (8 * b);
    }
    return f;
}

// the step into a stage's operand: codes at `lc` (swizzled rows of 128 B), scale bytes at `ls` (8 per row)
__device__ __forceinline__ void stash(const Fetch& f, uint8_t* lc, uint8_t* ls, int tid) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int chunk = tid + 256 * j, row = chunk >> 3;
        *(u4*)(lc + row * kRowBytes + (((chunk & 7) ^ (row & 7)) << 4)) = f.c[j];
    }
    *(uint32_t*)(ls + tid * 4) = f.s;
}

__device__ __forceinline__ float bias_at(const void* bias, int dtype, int64_t i) {
    if (dtype == AWQ_DTYPE_BF16) return load1<FmtBF16>(bias, i);
    if (dtype == AWQ_DTYPE_F16) return load1<FmtF16>(bias, i);
    return load1<FmtF32>(bias, i);
}

template <int OD>
__global__ __launch_bounds__(256) void mxfp4_gemm_kernel(const uint8_t* __restrict__ a_codes,
                                                         const uint8_t* __restrict__ a_scales, int64_t T,
                                                         const uint8_t* __restrict__ w_codes,
                                                         const uint8_t* __restrict__ w_scales, int64_t N, int64_t K,
                                                         const void* __restrict__ bias, int bias_dtype,
                                                         void* __restrict__ out, int64_t t_tiles, bool a_dwords,
                                                         bool w_dwords) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kStageBytes];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;   // the wave's 64 x 64 inside the tile
    const int64_t t0 = ((int64_t)blockIdx.x % t_tiles) * kTile, n0 = ((int64_t)blockIdx.x / t_tiles) * kTile;

    f16v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.0f;
    bool nan_a[2] = {false, false}, nan_w[2] = {false, false};

    Fetch fa = fetch(a_codes, a_scales, T, t0, K, 0, a_dwords, tid);
    Fetch fw = fetch(w_codes, w_scales, N, n0, K, 0, w_dwords, tid);
    stash(fa, lds, lds + 2 * kCodeBytes, tid);
    stash(fw, lds + kCodeBytes, lds + 2 * kCodeBytes + kScaleBytes, tid);
    __syncthreads();

    int stage = 0;
    for (int64_t k0 = 0; k0 < K; k0 += kStepK, stage ^= 1) {
        const bool more = k0 + kStepK < K;
        if (more) {
            fa = fetch(a_codes, a_scales, T, t0, K, k0 + kStepK, a_dwords, tid);
            fw = fetch(w_codes, w_scales, N, n0, K, k0 + kStepK, w_dwords, tid);
        }
        const uint8_t* la = lds + stage * kStageBytes;
        const uint8_t* lw = la + kCodeBytes;
        const uint8_t* sa = la + 2 * kCodeBytes;
        const uint8_t* sw = sa + kScaleBytes;
        uint64_t ea[2], ew[2];   // the 8 scale bytes of the lane's row in each instruction tile
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ea[i] = *(const uint64_t*)(sa + (wm + 32 * i + r) * 8);
            ew[i] = *(const uint64_t*)(sw + (wn + 32 * i + r) * 8);
        }
        const int slabs = (int)min((int64_t)4, (K - k0 + 63) / 64);
        for (int s = 0; s < slabs; ++s) {
            const int c = 2 * s + h;   // the lane's 16-B chunk = MX block of the step
            u4 qa[2], qw[2];
            int ba[2], bw[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int ra = wm + 32 * i + r, rw = wn + 32 * i + r;
                qa[i] = *(const u4*)(la + ra * kRowBytes + ((c ^ (ra & 7)) << 4));
                qw[i] = *(const u4*)(lw + rw * kRowBytes + ((c ^ (rw & 7)) << 4));
                ba[i] = (int)((ea[i] >> (8 * c)) & 0xFFu);
                bw[i] = (int)((ew[i] >> (8 * c)) & 0xFFu);
                nan_a[i] |= ba[i] == 255;
                nan_w[i] |= bw[i] == 255;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                        (i8v){(int)qa[i].x, (int)qa[i].y, (int)qa[i].z, (int)qa[i].w, 0, 0, 0, 0},
                        (i8v){(int)qw[j].x, (int)qw[j].y, (int)qw[j].z, (int)qw[j].w, 0, 0, 0, 0}, acc[i][j], 4, 4, 0,
                        ba[i], 0, bw[j]);
        }
        if (more) {
            uint8_t* na = lds + (stage ^ 1) * kStageBytes;
            stash(fa, na, na + 2 * kCodeBytes, tid);
            stash(fw, na + kCodeBytes, na + 2 * kCodeBytes + kScaleBytes, tid);
        }
        __syncthreads();
    }

    // a lane knows the flag of row / column l % 32 for its half of the k blocks; the result's rows are
    // spread over the registers, so the row flags travel as a ballot
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint64_t ma = __builtin_amdgcn_ballot_w64(nan_a[i]);
        const uint32_t row_nan = (uint32_t)ma | (uint32_t)(ma >> 32);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint64_t mw = __builtin_amdgcn_ballot_w64(nan_w[j]);
            const bool col_nan = ((((uint32_t)mw | (uint32_t)(mw >> 32)) >> r) & 1u) != 0u;
            const int64_t n = n0 + wn + 32 * j + r;
            if (n >= N) continue;
            const float b = bias ? bias_at(bias, bias_dtype, n) : 0.0f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = 8 * (v >> 2) + 4 * h + (v & 3);
                const int64_t t = t0 + wm + 32 * i + row;
                if (t >= T) continue;
                float y = bias ? acc[i][j][v] + b : acc[i][j][v];
                if (col_nan || ((row_nan >> row) & 1u)) y = __uint_as_float(0x7FC00000u);
                const int64_t o = t * N + n;
                if (OD == AWQ_DTYPE_F32) ((float*)out)[o] = y;
                else if (OD == AWQ_DTYPE_BF16) ((uint16_t*)out)[o] = (uint16_t)(__float_as_uint(rn_bf16(y)) >> 16);
                else ((_Float16*)out)[o] = (_Float16)y;
            }
        }
    }
}

bool float_dtype(int d) { return d == AWQ_DTYPE_BF16 || d == AWQ_DTYPE_F16 || d == AWQ_DTYPE_F32; }

}  // namespace
}  // namespace awq

using namespace awq;

extern "C" int awq_mxfp4_gemm(const uint8_t* a_codes, const uint8_t* a_scales, int64_t T, const uint8_t* w_codes,
                              const uint8_t* w_scales, int64_t N, int64_t K, const void* bias, int bias_dtype,
                              void* out, int out_dtype, void* stream) {
    if (T <= 0 || N <= 0 || K <= 0)
        return fail(AWQ_EINVAL, "awq_mxfp4_gemm: T, N and K must be positive (%lld, %lld, %lld)", (long long)T,
                    (long long)N, (long long)K);
    if (K % kBlockElems != 0)
        return fail(AWQ_EINVAL, "awq_mxfp4_gemm: K %% 32 must be 0, the MXFP4 block (K=%lld)", (long long)K);
    if (!float_dtype(out_dtype))
        return fail(AWQ_EINVAL, "awq_mxfp4_gemm: out dtype code %d is not bf16, fp16 or fp32", out_dtype);
    if (bias && !float_dtype(bias_dtype))
        return fail(AWQ_EINVAL, "awq_mxfp4_gemm: bias dtype code %d is not bf16, fp16 or fp32", bias_dtype);
    const int64_t lim = (int64_t)1 << 60, t_tiles = (T + kTile - 1) / kTile, n_tiles = (N + kTile - 1) / kTile;
    if (K > lim / T || K > lim / N || N > lim / T || t_tiles > (int64_t)0x7FFFFFFF / n_tiles)
        return fail(AWQ_EUNSUPPORTED, "awq_mxfp4_gemm: %lld x %lld x %lld exceeds 2^60 elements or 2^31 - 1 tiles",
                    (long long)T, (long long)N, (long long)K);
    if (!a_codes || !a_scales || !w_codes || !w_scales || !out)
        return fail(AWQ_EINVAL, "awq_mxfp4_gemm: null argument");
    const size_t oe = out_dtype == AWQ_DTYPE_F32 ? 4 : 2;
    if (!aligned(a_codes, 16) || !aligned(w_codes, 16) || !aligned(out, oe) ||
        !aligned(bias, bias_dtype == AWQ_DTYPE_F32 ? 4 : 2))
        return fail(AWQ_EINVAL, "awq_mxfp4_gemm: codes need 16-B alignment, out and bias their element's");
    const bool quads = K / kBlockElems % 4 == 0;
    const bool a_dwords = quads && aligned(a_scales, 4), w_dwords = quads && aligned(w_scales, 4);
    const dim3 grid((unsigned)(t_tiles * n_tiles));
#define AWQ_MX(OD) \
    hipLaunchKernelGGL((mxfp4_gemm_kernel<OD>), grid, dim3(256), 0, (hipStream_t)stream, a_codes, a_scales, T, w_codes, \
                       w_scales, N, K, bias, bias_dtype, out, t_tiles, a_dwords, w_dwords)
    if (out_dtype == AWQ_DTYPE_BF16) AWQ_MX(AWQ_DTYPE_BF16);
    else if (out_dtype == AWQ_DTYPE_F16) AWQ_MX(AWQ_DTYPE_F16);
    else AWQ_MX(AWQ_DTYPE_F32);
#undef AWQ_MX
    return hip_status(hipPeekAtLastError(), "awq mxfp4 gemm kernel");
}
