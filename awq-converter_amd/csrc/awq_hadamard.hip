// awq_hadamard.hip — awq_hadamard_rows / awq_hadamard_cols (include/awq_hip.h): the
// fast Walsh-Hadamard transform of a weight matrix along either axis, out_seg = (in_seg * pre) (M (x)
// H_{2^k}) / sqrt(L) per L-segment, L = m 2^k.  Additions and subtractions only (plus m fused
// multiply-adds by +-1 per element where m > 1), in fp32 for fp32 matrices and in fp64 for 16-bit ones
// (Arith below says why), one rounding into the dtype.
//
// The index of an element inside its segment is i = j P + p (P = 2^k, j < m).  The Sylvester factor
// works on the bits of p, the mix M on j; the factors commute, so every stage is taken where the
// bit it works on lives.
//
// Rows ([R, K], segments are contiguous: the matrix is a flat sequence of R K / L segments).  A lane
// owns 8-element chunks (one 16-B load of 16-bit data, two of fp32); chunk c = j P/8 + q of a segment.
//   bits 0..2 of p   the lane's own 8 registers                        (3 stages, no data movement)
//   bits 3..8        the 64 lanes of a wave: lane ^ 1, ^ 2 by DPP quad_perm, ^ 4, ^ 8 by ds_swizzle
//                    (no LDS memory), ^ 16, ^ 32 by v_permlane16_swap / v_permlane32_swap
//   bits 9, 10       the 2 or 4 waves of the workgroup: ONE LDS exchange — every lane writes its
//                    registers, and after the barrier adds the 2 or 4 waves' values of its own slot
//                    with the signs of H_2 / H_4
//   bits 11..13      QR = 2, 4, 8 chunks per lane (registers again)
//   j                m chunks per lane, one per j: out[j'] = sum_j M[j][j'] x[j], a run-time loop over
//                    j' with the column of M read from LDS (broadcast), fused with the store
// A segment of up to 512 elements lives in (a part of) one wave, and a one-wave workgroup carries
// 64 / (P / 8) of them (the head pass: 8 segments of 64 per wave); 1024 elements take 2 waves, 2048
// and more 4 waves with QR chunks per lane (16384: 8 chunks = 64 registers).  m > 1: P <= 1024, the
// lane holds 8 m values (m = 28: 224 VGPRs, one wave per SIMD).
//
// Columns ([K, N], down the rows).  A lane owns a 16-B strip of 8 consecutive columns (fp32: 32 B),
// whose 8 values never meet: every stage pairs whole strips of two rows.  One pass transforms ONE
// factor of L over a view [A, Lk, Wd] of the matrix (Wd = inner * N):
//   power-of-two factor Lk = 16 NR (NR = 1, 2, 4, 8):  a 256-thread workgroup owns Lk rows x 16
//       strips (256 B of a row, consecutive lanes: coalesced).  Row i = 16 rr + y: rr in the lane's
//       NR registers, y bits 0, 1 = lane bits 4, 5 (permlane swaps), y bits 2, 3 = the wave (the LDS
//       exchange above).
//   mix factor Lk = m:  a lane owns its strip of all m rows (registers), the j' loop as above.
// L = m P takes the passes (m), then P itself if P <= 128, else (P / b) and (b), b = min(128, P / 16):
// one pass up to L = 128 (the head pass, small hidden sizes), two for every larger power of two up
// to 16384 and for m 2^k with 2^k <= 128, three for m 256 .. m 1024.  Between passes the values
// stay in the arithmetic type: fp64 in the caller's workspace for a 16-bit matrix, fp32 in `out`
// itself for an fp32 one; every pass after the first works in place on it: a workgroup loads its whole tile before the barrier and stores after it, and tiles
// are disjoint.  pre is applied by the first pass, 1 / sqrt(L) by the last.
#include <type_traits>

#include "awq_lanes.h"

namespace awq {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t w4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int kMaxL = 16384;
constexpr int kColStrips = 16;          // strips (of 8 columns) per power-of-two column tile
constexpr int kMixStrips = 256;         // strips per mix column tile: one per thread

struct CodeBF16 {
    static __device__ __forceinline__ float dec(uint32_t h) { return __uint_as_float(h << 16); }
    static __device__ __forceinline__ uint32_t enc(float f) {
        if (f != f) return 0x7FC0u;
        const uint32_t u = __float_as_uint(f);
        return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    }
};
struct CodeF16 {
    static __device__ __forceinline__ float dec(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }
    static __device__ __forceinline__ uint32_t enc(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
};

// The arithmetic type of a matrix dtype.  fp32 matrices: float (the error of log2 L + m float
// additions is a few 2^-24 of the segment's norm, far below the output's own ulp wherever it
// matters to an fp32 reader).  16-bit matrices: double — an output that cancels to nearly zero has
// a 16-bit ulp far below the float error of its sum (fp16 keeps ulps of 2^-24 absolute, bf16 8
// relative bits at any magnitude), and only the sum carried past float's 24 bits rounds to the
// 16-bit value of the exact result.  16-bit inputs times an fp32 pre are exact in double, and so
// are nearly all the sums (at most 11 + 24 + log2 L + 5 bits apart from the inputs' exponent range).
template <int DT> struct Arith { typedef double T; };
template <> struct Arith<AWQ_DTYPE_F32> { typedef float T; };
constexpr int kDtypeF64 = 64;           // the workspace of a 16-bit column transform (never a caller's dtype)

// double -> float rounded to odd: the 16-bit RNE rounding that follows is then the rounding of the
// double itself (float keeps 13 / 16 bits more than the target, so the sticky bit is enough)
__device__ __forceinline__ float narrow(double x) {
    const float f = (float)x;
    const double d = (double)f;
    if (d == x || d != d) return f;
    uint32_t u = __float_as_uint(f);
    if (__builtin_fabs(d) > __builtin_fabs(x)) --u;      // towards zero (f is not zero here: |d| > |x| >= 0)
    return __uint_as_float(u | 1u);
}

// 8 consecutive elements at p (16-B aligned), in the arithmetic type and back (one RNE rounding)
template <int DT> struct Elem {
    typedef typename std::conditional<DT == AWQ_DTYPE_BF16, CodeBF16, CodeF16>::type C;
    static constexpr int kBytes = 2;
    template <typename T>
    static __device__ __forceinline__ void load8(const char* p, T (&x)[8]) {
        const w4 v = __builtin_nontemporal_load((const w4*)p);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = (T)C::dec(v[i] & 0xFFFFu);
            x[2 * i + 1] = (T)C::dec(v[i] >> 16);
        }
    }
    template <typename T>
    static __device__ __forceinline__ void store8(char* p, const T (&x)[8]) {
        w4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = C::enc(narrow(x[2 * i])) | (C::enc(narrow(x[2 * i + 1])) << 16);
        __builtin_nontemporal_store(v, (w4*)p);
    }
};
template <> struct Elem<AWQ_DTYPE_F32> {
    static constexpr int kBytes = 4;
    template <typename T>
    static __device__ __forceinline__ void load8(const char* p, T (&x)[8]) {
        const f4 a = __builtin_nontemporal_load((const f4*)p), b = __builtin_nontemporal_load((const f4*)p + 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) { x[i] = (T)a[i]; x[4 + i] = (T)b[i]; }
    }
    template <typename T>
    static __device__ __forceinline__ void store8(char* p, const T (&x)[8]) {
        __builtin_nontemporal_store((f4){(float)x[0], (float)x[1], (float)x[2], (float)x[3]}, (f4*)p);
        __builtin_nontemporal_store((f4){(float)x[4], (float)x[5], (float)x[6], (float)x[7]}, (f4*)p + 1);
    }
};
template <> struct Elem<kDtypeF64> {
    static constexpr int kBytes = 8;
    static __device__ __forceinline__ void load8(const char* p, double (&x)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const d2 a = __builtin_nontemporal_load((const d2*)p + i);
            x[2 * i] = a[0];
            x[2 * i + 1] = a[1];
        }
    }
    static __device__ __forceinline__ void store8(char* p, const double (&x)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) __builtin_nontemporal_store((d2){x[2 * i], x[2 * i + 1]}, (d2*)p + i);
    }
};

// the three stages inside a chunk
template <typename T>
__device__ __forceinline__ void chunk_stages(T (&x)[8]) {
#pragma unroll
    for (int s = 1; s < 8; s <<= 1)
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (!(i & s)) {
                const T a = x[i], b = x[i + s];
                x[i] = a + b;
                x[i + s] = a - b;
            }
}

// one stage between lanes l and l ^ (1 << B): the lower lane keeps own + partner, the upper one
// partner - own (upper = bit B of the lane)
// (a double moves as its two 32-bit halves)
template <int B>
__device__ __forceinline__ float lane_stage(float v, bool upper) {
    if constexpr (B < 4) {
        float p;
        if constexpr (B == 0) p = dpp_mov<0xB1>(v);           // quad_perm [1,0,3,2]
        else if constexpr (B == 1) p = dpp_mov<0x4E>(v);      // quad_perm [2,3,0,1]
        else p = __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x1F | ((1 << B) << 10)));
        return (upper ? -v : v) + p;
    } else {
        float a, b;                                            // the lower / the upper half's value
        if constexpr (B == 4) swap16(v, a, b); else swap32(v, a, b);
        return upper ? a - b : a + b;
    }
}
__device__ __forceinline__ double join(uint32_t lo, uint32_t hi) {
    return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}
template <int B>
__device__ __forceinline__ double lane_stage(double v, bool upper) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)u, hi = (uint32_t)(u >> 32);
    if constexpr (B < 4) {
        uint32_t pl, ph;
        if constexpr (B == 0) { pl = dpp_mov<0xB1>(lo); ph = dpp_mov<0xB1>(hi); }
        else if constexpr (B == 1) { pl = dpp_mov<0x4E>(lo); ph = dpp_mov<0x4E>(hi); }
        else {
            pl = (uint32_t)__builtin_amdgcn_ds_swizzle((int)lo, 0x1F | ((1 << B) << 10));
            ph = (uint32_t)__builtin_amdgcn_ds_swizzle((int)hi, 0x1F | ((1 << B) << 10));
        }
        return (upper ? -v : v) + join(pl, ph);
    } else {
        uint32_t al, bl, ah, bh;
        if constexpr (B == 4) { swap16(lo, al, bl); swap16(hi, ah, bh); } else { swap32(lo, al, bl); swap32(hi, ah, bh); }
        const double a = join(al, ah), b = join(bl, bh);
        return upper ? a - b : a + b;
    }
}
template <int B, typename T, int NR>
__device__ __forceinline__ void lane_stage_all(T (&x)[NR][8], int lane) {
    const bool upper = (lane >> B) & 1;
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int e = 0; e < 8; ++e) x[r][e] = lane_stage<B>(x[r][e], upper);
}

// stages between the registers of a lane: rows r and r + s * STEP for s = 1, 2, .. < N
template <int N, int STEP, typename T, int NR>
__device__ __forceinline__ void row_stages(T (&x)[NR][8]) {
#pragma unroll
    for (int s = 1; s < N; s <<= 1)
#pragma unroll
        for (int r = 0; r < N; ++r)
            if (!(r & s))
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const T a = x[r * STEP][e], b = x[(r + s) * STEP][e];
                    x[r * STEP][e] = a + b;
                    x[(r + s) * STEP][e] = a - b;
                }
}

// the stages between the NW waves of a workgroup: slot (r, part, lane) of every wave through LDS, then
// sum_w' (-1)^popc(w & w') value[w'] in ascending w'.  A slot is 16 B (4 floats or 2 doubles), RB
// rows go through per exchange (doubles: 4 at a time past 4 rows, so that the buffer is never
// larger than the float one), xch holds NW * RB * (8 / per slot) * 64 slots.
template <typename T> struct Slot {
    static constexpr int kPer = 16 / sizeof(T);                                     // values per slot
    static constexpr int kParts = 8 / kPer;                                         // slots per chunk
    typedef T V __attribute__((ext_vector_type(kPer)));
    static constexpr int batch(int NR) { return sizeof(T) == 8 && NR > 4 ? 4 : NR; }
    static constexpr int slots(int NW, int NR) { return NW * batch(NR) * kParts * 64; }
};
template <int NW, typename T, int NR>
__device__ __forceinline__ void wave_stages(T (&x)[NR][8], typename Slot<T>::V* xch, int w, int lane) {
    typedef typename Slot<T>::V V;
    constexpr int PER = Slot<T>::kPer, PARTS = Slot<T>::kParts, RB = Slot<T>::batch(NR);
    static_assert(NR % RB == 0, "rows per exchange");
#pragma unroll
    for (int r0 = 0; r0 < NR; r0 += RB) {
        if (r0) __syncthreads();                                                     // the batch before has been read
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int h = 0; h < PARTS; ++h) {
                V v;
#pragma unroll
                for (int i = 0; i < PER; ++i) v[i] = x[r0 + r][PER * h + i];
                xch[((w * RB + r) * PARTS + h) * 64 + lane] = v;
            }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int h = 0; h < PARTS; ++h) {
                V acc = xch[(r * PARTS + h) * 64 + lane];
#pragma unroll
                for (int wp = 1; wp < NW; ++wp) {
                    const V v = xch[((wp * RB + r) * PARTS + h) * 64 + lane];
                    acc = (__builtin_popcount(w & wp) & 1) ? acc - v : acc + v;
                }
#pragma unroll
                for (int i = 0; i < PER; ++i) x[r0 + r][PER * h + i] = acc[i];
            }
    }
}

// smix[j' * M + j] = mix[j * M + j']: the column of M an output block j' needs, contiguous
template <int M>
__device__ __forceinline__ void stage_mix(const float* __restrict__ mix, float* smix, int t, int nt) {
    for (int i = t; i < M * M; i += nt) smix[(i % M) * M + i / M] = mix[i];
    __syncthreads();
}
template <int M, typename T>
__device__ __forceinline__ void mix_block(const T (&x)[M][8], const float* smix, int jp, T scale, T (&y)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const T c = (T)smix[jp * M + j];
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = __builtin_elementwise_fma(c, x[j][e], y[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] *= scale;
}

// ---------------------------------------------------------------- rows
// NW == 1: one wave, P / 8 = 2^lgpc <= 64 lanes per segment, 64 >> lgpc segments per wave
// NW > 1: one segment per workgroup of 64 NW threads, P / 8 = 64 NW QR
template <int DT, int M, int QR, int NW>
__global__ __launch_bounds__(64 * NW) void hadamard_rows_kernel(const char* __restrict__ in, char* __restrict__ out,
                                                                const float* __restrict__ pre,
                                                                const float* __restrict__ mix, int64_t nseg,
                                                                uint32_t segs_per_row, int lgpc, double scale_) {
    typedef Elem<DT> E;
    typedef typename Arith<DT>::T T;
    constexpr int NR = M * QR;
    static_assert(M == 1 || QR == 1, "chunks per lane: m or QR");
    __shared__ typename Slot<T>::V xch[NW > 1 ? Slot<T>::slots(NW, NR) : 1];
    const T scale = (T)scale_;
    __shared__ float smix[M > 1 ? M * M : 1];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t pc = 1u << lgpc;
    const uint32_t tps = NW > 1 ? 64u * NW : pc;           // threads per segment
    const uint32_t q0 = NW > 1 ? (uint32_t)t : ((uint32_t)t & (tps - 1));
    const int64_t seg = NW > 1 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (64 >> lgpc) + (t >> lgpc);
    const bool live = seg < nseg;
    const int64_t sc = live ? seg : nseg - 1;              // (a lane past the end reads the last segment and stores nothing)
    const int64_t L = (int64_t)M * pc * 8;
    const int64_t base = sc * L;
    const uint32_t pbase = (uint32_t)(sc % segs_per_row) * (uint32_t)L;
    if constexpr (M > 1) stage_mix<M>(mix, smix, t, 64 * NW);

    T x[NR][8];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const uint32_t c = (uint32_t)(r / QR) * pc + (uint32_t)(r % QR) * tps + q0;
        E::load8(in + (base + 8 * (int64_t)c) * E::kBytes, x[r]);
        if (pre) {
            const f4 a = *(const f4*)(pre + pbase + 8 * c), b = *(const f4*)(pre + pbase + 8 * c + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) { x[r][i] *= (T)a[i]; x[r][4 + i] *= (T)b[i]; }
        }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) chunk_stages(x[r]);
    const int nl = NW > 1 ? 6 : lgpc;                      // stages between lanes (wave-uniform)
    if (nl > 0) lane_stage_all<0>(x, lane);
    if (nl > 1) lane_stage_all<1>(x, lane);
    if (nl > 2) lane_stage_all<2>(x, lane);
    if (nl > 3) lane_stage_all<3>(x, lane);
    if (nl > 4) lane_stage_all<4>(x, lane);
    if (nl > 5) lane_stage_all<5>(x, lane);
    if constexpr (NW > 1) wave_stages<NW>(x, xch, w, lane);
    if constexpr (QR > 1) row_stages<QR, 1>(x);

    if constexpr (M == 1) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[r][e] *= scale;
            if (live) E::store8(out + (base + 8 * (int64_t)((uint32_t)r * tps + q0)) * E::kBytes, x[r]);
        }
    } else {
#pragma unroll 1
        for (int jp = 0; jp < M; ++jp) {
            T y[8];
            mix_block<M>(x, smix, jp, scale, y);
            if (live) E::store8(out + (base + 8 * (int64_t)((uint32_t)jp * pc + q0)) * E::kBytes, y);
        }
    }
}

// ---------------------------------------------------------------- columns
// the view [A, Lk, Wd]; pre (first pass only) is indexed by the matrix row (a Lk + i) inner + col / N
template <int DI, int DO, int NR>
__global__ __launch_bounds__(256) void hadamard_cols_kernel(const char* in, char* out, const float* __restrict__ pre,
                                                            int64_t Wd, uint32_t tiles_x, int64_t N, int64_t inner,
                                                            double scale_) {
    typedef Elem<DI> EI;
    typedef Elem<DO> EO;
    typedef typename std::conditional<DI == AWQ_DTYPE_F32 && DO == AWQ_DTYPE_F32, float, double>::type T;
    constexpr int Lk = 16 * NR;
    __shared__ typename Slot<T>::V xch[Slot<T>::slots(4, NR)];
    const T scale = (T)scale_;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int y = (lane >> 4) | (w << 2);
    const int64_t a = blockIdx.x / tiles_x;
    const int64_t col = (int64_t)(blockIdx.x % tiles_x) * (8 * kColStrips) + 8 * (lane & 15);
    const bool live = col < Wd;
    const int64_t cc = live ? col : 0;                     // (a lane past the edge reads strip 0 and stores nothing)
    const int64_t row0 = a * Lk + y;
    const int64_t prow = pre ? cc / N : 0;

    T x[NR][8];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int64_t g = row0 + 16 * r;
        EI::load8(in + (g * Wd + cc) * EI::kBytes, x[r]);
        if (pre) {
            const T p = (T)pre[g * inner + prow];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[r][e] *= p;
        }
    }
    lane_stage_all<4>(x, lane);
    lane_stage_all<5>(x, lane);
    wave_stages<4>(x, xch, w, lane);
    if constexpr (NR > 1) row_stages<NR, 1>(x);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[r][e] *= scale;
        if (live) EO::store8(out + ((row0 + 16 * r) * Wd + cc) * EO::kBytes, x[r]);
    }
}

// the mix factor: Lk = M rows, a lane's strip of all of them; writes the workspace's type (fp32 for an
// fp32 matrix, fp64 for a 16-bit one)
template <int DI, int M>
__global__ __launch_bounds__(256) void hadamard_cols_mix_kernel(const char* in, char* out, const float* __restrict__ pre,
                                                                const float* __restrict__ mix, int64_t Wd,
                                                                uint32_t tiles_x, int64_t N, int64_t inner, double scale_) {
    typedef Elem<DI> EI;
    typedef Elem<DI == AWQ_DTYPE_F32 ? AWQ_DTYPE_F32 : kDtypeF64> EO;
    typedef typename Arith<DI>::T T;
    __shared__ float smix[M * M];
    const T scale = (T)scale_;
    const int t = threadIdx.x;
    const int64_t a = blockIdx.x / tiles_x;
    const int64_t col = (int64_t)(blockIdx.x % tiles_x) * (8 * kMixStrips) + 8 * t;
    const bool live = col < Wd;
    const int64_t cc = live ? col : 0;
    const int64_t prow = pre ? cc / N : 0;
    stage_mix<M>(mix, smix, t, 256);
    T x[M][8];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int64_t g = a * M + j;
        EI::load8(in + (g * Wd + cc) * EI::kBytes, x[j]);
        if (pre) {
            const T p = (T)pre[g * inner + prow];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[j][e] *= p;
        }
    }
#pragma unroll 1
    for (int jp = 0; jp < M; ++jp) {
        T y[8];
        mix_block<M>(x, smix, jp, scale, y);
        if (live) EO::store8(out + ((a * M + jp) * Wd + cc) * EO::kBytes, y);
    }
}

// ---------------------------------------------------------------- launches
struct RowsArgs {
    const char* in; char* out; const float* pre; const float* mix;
    int64_t nseg; uint32_t segs_per_row; int lgpc; double scale; hipStream_t stream;
};
template <int DT, int M, int QR, int NW>
hipError_t launch_rows_as(const RowsArgs& a) {
    const int64_t grid = NW > 1 ? a.nseg : (a.nseg + (64 >> a.lgpc) - 1) / (64 >> a.lgpc);
    hipLaunchKernelGGL((hadamard_rows_kernel<DT, M, QR, NW>), dim3((unsigned)grid), dim3(64 * NW), 0, a.stream, a.in,
                       a.out, a.pre, a.mix, a.nseg, a.segs_per_row, a.lgpc, a.scale);
    return hipPeekAtLastError();
}
template <int DT>
hipError_t launch_rows(const RowsArgs& a, int m) {
    const int pc = 1 << a.lgpc;
    if (m == 1) {
        if (pc <= 64) return launch_rows_as<DT, 1, 1, 1>(a);
        if (pc == 128) return launch_rows_as<DT, 1, 1, 2>(a);
        if (pc == 256) return launch_rows_as<DT, 1, 1, 4>(a);
        if (pc == 512) return launch_rows_as<DT, 1, 2, 4>(a);
        if (pc == 1024) return launch_rows_as<DT, 1, 4, 4>(a);
        return launch_rows_as<DT, 1, 8, 4>(a);
    }
    if (pc == 128) return launch_rows_as<DT, 12, 1, 2>(a);           // 12 * 1024: the one m > 1 length past a wave
    if (m == 12) return launch_rows_as<DT, 12, 1, 1>(a);
    if (m == 20) return launch_rows_as<DT, 20, 1, 1>(a);
    return launch_rows_as<DT, 28, 1, 1>(a);
}

struct ColsArgs {
    const char* in; char* out; const float* pre; const float* mix;
    int64_t A, Wd, N, inner; double scale; hipStream_t stream;
};
template <int DI, int DO>
hipError_t launch_cols_pow2(const ColsArgs& a, int Lk) {
    const int64_t tx = (a.Wd + 8 * kColStrips - 1) / (8 * kColStrips);
    const dim3 grid((unsigned)(a.A * tx)), block(256);
#define AWQ_HAD_COLS(NR)                                                                                              \
    hipLaunchKernelGGL((hadamard_cols_kernel<DI, DO, NR>), grid, block, 0, a.stream, a.in, a.out, a.pre, a.Wd,       \
                       (uint32_t)tx, a.N, a.inner, a.scale)
    if (Lk == 16) AWQ_HAD_COLS(1);
    else if (Lk == 32) AWQ_HAD_COLS(2);
    else if (Lk == 64) AWQ_HAD_COLS(4);
    else AWQ_HAD_COLS(8);
#undef AWQ_HAD_COLS
    return hipPeekAtLastError();
}
template <int DI>
hipError_t launch_cols_mix(const ColsArgs& a, int m) {
    const int64_t tx = (a.Wd + 8 * kMixStrips - 1) / (8 * kMixStrips);
    const dim3 grid((unsigned)(a.A * tx)), block(256);
#define AWQ_HAD_MIX(M)                                                                                                \
    hipLaunchKernelGGL((hadamard_cols_mix_kernel<DI, M>), grid, block, 0, a.stream, a.in, a.out, a.pre, a.mix, a.Wd, \
                       (uint32_t)tx, a.N, a.inner, a.scale)
    if (m == 12) AWQ_HAD_MIX(12);
    else if (m == 20) AWQ_HAD_MIX(20);
    else AWQ_HAD_MIX(28);
#undef AWQ_HAD_MIX
    return hipPeekAtLastError();
}
// one pass: factor Lk of the view [A, Lk, inner * N]; is_mix: the m x m factor
hipError_t launch_cols_pass(const ColsArgs& a, int di, int dq, int Lk, bool is_mix) {
    if (is_mix) {
        if (di == AWQ_DTYPE_BF16) return launch_cols_mix<AWQ_DTYPE_BF16>(a, Lk);
        if (di == AWQ_DTYPE_F16) return launch_cols_mix<AWQ_DTYPE_F16>(a, Lk);
        return launch_cols_mix<AWQ_DTYPE_F32>(a, Lk);
    }
    if (di == AWQ_DTYPE_F32) return launch_cols_pow2<AWQ_DTYPE_F32, AWQ_DTYPE_F32>(a, Lk);
    if (di == kDtypeF64) {
        if (dq == AWQ_DTYPE_BF16) return launch_cols_pow2<kDtypeF64, AWQ_DTYPE_BF16>(a, Lk);
        if (dq == AWQ_DTYPE_F16) return launch_cols_pow2<kDtypeF64, AWQ_DTYPE_F16>(a, Lk);
        return launch_cols_pow2<kDtypeF64, kDtypeF64>(a, Lk);
    }
    if (di == AWQ_DTYPE_BF16) {
        if (dq == AWQ_DTYPE_BF16) return launch_cols_pow2<AWQ_DTYPE_BF16, AWQ_DTYPE_BF16>(a, Lk);
        return launch_cols_pow2<AWQ_DTYPE_BF16, kDtypeF64>(a, Lk);
    }
    if (dq == AWQ_DTYPE_F16) return launch_cols_pow2<AWQ_DTYPE_F16, AWQ_DTYPE_F16>(a, Lk);
    return launch_cols_pow2<AWQ_DTYPE_F16, kDtypeF64>(a, Lk);
}

// the factors of a column transform, most significant digit of the row index first
struct ColsPlan { int n; int len[3]; bool is_mix[3]; };
ColsPlan plan_cols(int64_t L, int m) {
    ColsPlan p{0, {0, 0, 0}, {false, false, false}};
    const int P = (int)(L / m);
    if (m > 1) { p.len[p.n] = m; p.is_mix[p.n++] = true; }
    if (P <= 128) p.len[p.n++] = P;
    else {
        const int b = P / 16 < 128 ? P / 16 : 128;
        p.len[p.n++] = P / b;
        p.len[p.n++] = b;
    }
    return p;
}

// the checks both entries share; 0, or the failure's code (the message is set)
int check_transform(const char* what, int dtype, int64_t L, int m, const float* mix) {
    if (dtype != AWQ_DTYPE_BF16 && dtype != AWQ_DTYPE_F16 && dtype != AWQ_DTYPE_F32)
        return fail(AWQ_EUNSUPPORTED, "%s takes bf16 / fp16 / fp32 matrices (dtype code %d)", what, dtype);
    if (m != 1 && m != 12 && m != 20 && m != 28)
        return fail(AWQ_EUNSUPPORTED, "%s: the mix order m must be 1, 12, 20 or 28 (m=%d)", what, m);
    if (L <= 0 || L % m != 0) return fail(AWQ_EINVAL, "%s: L must be a positive multiple of m (L=%lld, m=%d)", what, (long long)L, m);
    const int64_t P = L / m;
    if ((P & (P - 1)) != 0 || P < 16)
        return fail(AWQ_EINVAL, "%s: L / m must be a power of two, 2^k >= 16 (L=%lld, m=%d)", what, (long long)L, m);
    if (L > kMaxL) return fail(AWQ_EUNSUPPORTED, "%s: L is limited to %d (L=%lld)", what, kMaxL, (long long)L);
    if (m > 1 && !mix) return fail(AWQ_EINVAL, "%s: m > 1 needs the mix matrix (m=%d, mix is null)", what, m);
    return AWQ_OK;
}

}  // namespace
}  // namespace awq

extern "C" int awq_hadamard_rows(const void* in, int dtype, int64_t R, int64_t K, int64_t L, int m, const float* pre,
                                 const float* mix, void* out, void* stream) {
    using namespace awq;
    set_error(AWQ_OK, "");
    if (R < 0 || K < 0) return fail(AWQ_EINVAL, "negative size (R=%lld, K=%lld)", (long long)R, (long long)K);
    if (const int rc = check_transform("awq_hadamard_rows", dtype, L, m, mix)) return rc;
    if (K % L != 0) return fail(AWQ_EINVAL, "awq_hadamard_rows: L must divide K (K=%lld, L=%lld)", (long long)K, (long long)L);
    if (R == 0 || K == 0) return AWQ_OK;
    const int64_t spr = K / L, pc = L / m / 8, per = pc < 64 ? 64 / pc : 1;   // segments per row / per workgroup
    if (K >= ((int64_t)1 << 31) || R >= ((int64_t)1 << 31) || (R * spr + per - 1) / per >= ((int64_t)1 << 31))
        return fail(AWQ_EUNSUPPORTED, "awq_hadamard_rows: R and K are limited to 2^31 - 1 and the grid to 2^31 - 1 "
                                      "workgroups (R=%lld, K=%lld)", (long long)R, (long long)K);
    if (!in || !out) return fail(AWQ_EINVAL, "null argument");
    if (!aligned(in, 16) || !aligned(out, 16) || !aligned(pre, 16) || !aligned(mix, 4))
        return fail(AWQ_EINVAL, "misaligned argument (in, out and pre need 16-B alignment)");
    int lgpc = 0;
    while ((8 << lgpc) < L / m) ++lgpc;
    const RowsArgs a{(const char*)in, (char*)out, pre, mix, R * (K / L), (uint32_t)(K / L), lgpc,
                     1.0 / __builtin_sqrt((double)L), (hipStream_t)stream};
    hipError_t e;
    if (dtype == AWQ_DTYPE_BF16) e = launch_rows<AWQ_DTYPE_BF16>(a, m);
    else if (dtype == AWQ_DTYPE_F16) e = launch_rows<AWQ_DTYPE_F16>(a, m);
    else e = launch_rows<AWQ_DTYPE_F32>(a, m);
    return hip_status(e, "awq hadamard rows kernel");
}

extern "C" int64_t awq_hadamard_cols_work_bytes(int dtype, int64_t K, int64_t N, int64_t L, int m) {
    using namespace awq;
    if (K <= 0 || N <= 0 || L <= 0 || (m != 1 && m != 12 && m != 20 && m != 28) || L % m != 0 || L / m < 16 || L > kMaxL)
        return 0;
    if (dtype == AWQ_DTYPE_F32 || plan_cols(L, m).n == 1) return 0;
    return K * N * 8;
}

extern "C" int awq_hadamard_cols(const void* in, int dtype, int64_t K, int64_t N, int64_t L, int m, const float* pre,
                                 const float* mix, void* out, void* work, void* stream) {
    using namespace awq;
    set_error(AWQ_OK, "");
    if (K < 0 || N < 0) return fail(AWQ_EINVAL, "negative size (K=%lld, N=%lld)", (long long)K, (long long)N);
    if (const int rc = check_transform("awq_hadamard_cols", dtype, L, m, mix)) return rc;
    if (K % L != 0) return fail(AWQ_EINVAL, "awq_hadamard_cols: L must divide K (K=%lld, L=%lld)", (long long)K, (long long)L);
    if (N % 8 != 0) return fail(AWQ_EINVAL, "awq_hadamard_cols: N %% 8 must be 0 (N=%lld)", (long long)N);
    if (K == 0 || N == 0) return AWQ_OK;
    // the widest grid is the last power-of-two pass': K / 16 row blocks x ceil(N / 128) tiles
    if (K >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31) || (K / 16) * ((N + 127) / 128 + 1) >= ((int64_t)1 << 31))
        return fail(AWQ_EUNSUPPORTED, "awq_hadamard_cols: K and N are limited to 2^31 - 1 and the grid to 2^31 - 1 "
                                      "workgroups (K=%lld, N=%lld)", (long long)K, (long long)N);
    if (!in || !out) return fail(AWQ_EINVAL, "null argument");
    const ColsPlan plan = plan_cols(L, m);
    void* tmp = dtype == AWQ_DTYPE_F32 ? out : work;
    if (plan.n > 1 && !tmp)
        return fail(AWQ_EINVAL, "awq_hadamard_cols: L=%lld takes %d passes and needs the workspace "
                                "(awq_hadamard_cols_work_bytes)", (long long)L, plan.n);
    if (!aligned(in, 16) || !aligned(out, 16) || !aligned(work, 16) || !aligned(pre, 4) || !aligned(mix, 4))
        return fail(AWQ_EINVAL, "misaligned argument (in, out and work need 16-B alignment)");
    int64_t A = K / L, inner = L;
    for (int p = 0; p < plan.n; ++p) {
        const bool first = p == 0, last = p == plan.n - 1;
        inner /= plan.len[p];
        const ColsArgs a{(const char*)(first ? in : tmp), (char*)(last ? out : tmp), first ? pre : nullptr, mix,
                         A, inner * N, N, inner, last ? 1.0 / __builtin_sqrt((double)L) : 1.0,
                         (hipStream_t)stream};
        const int between = dtype == AWQ_DTYPE_F32 ? AWQ_DTYPE_F32 : kDtypeF64;
        const hipError_t e = launch_cols_pass(a, first ? dtype : between, last ? dtype : between, plan.len[p],
                                              plan.is_mix[p]);
        if (e != hipSuccess) return hip_status(e, "awq hadamard cols kernel");
        A *= plan.len[p];
    }
    return AWQ_OK;
}
