/*
 * awq_hip.h — C ABI of libawq_hip.so, the MI355X (gfx950) group quantizer.
 *
 * The reference (shanefitch/AWQ-Converter) has no FFI: its hot path is the Python
 * method AWQQuantizer._quantize_per_group (src/awq_quantizer/quantization/awq.py:286-374),
 * reached from AWQQuantizer.quantize (awq.py:376-433) and from the CLI's
 * quantize_tensor_batch (src/awq_quantizer/main.py:374).  These entry points replace
 * that method's arithmetic; the drop-in Python class (awq-converter_amd/awq_quantizer/
 * quantization/awq.py) binds them with ctypes.  See INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes; every pointer argument is DEVICE memory allocated by the
 *     caller unless stated otherwise; the library never allocates or frees device memory
 *     and keeps no global mutable state (re-entrant; one stream per call);
 *   - `stream` is a hipStream_t (NULL = legacy default stream); launches are asynchronous
 *     on that stream, nothing synchronises (pinned per entry point, memsets and later stages
 *     included, by tests/test_stream_order_gpu.py; re-entrancy by tests/test_reentrancy_host.py);
 *   - return 0 on success, an AWQ_E* code otherwise; awq_last_error() (thread-local)
 *     then holds a message.  Invalid arguments are reported before anything is launched.
 *
 * Layout: the input is [rows, K] row-major (the reference's dim 0 = rows, remaining dims
 * flattened = K, awq.py:306-320).  Groups are `group_size` consecutive elements along K;
 * a tail group shorter than group_size is zero-padded for its min/max (awq.py:337-339).
 * G = ceil(K / group_size).
 *
 * Outputs (each may be NULL when not wanted; at least one must be non-NULL):
 *   scales    fp16 bits [rows, G]            (awq.py:411, value = fp16(scale))
 *   zeros     int32     [rows, G]            (awq.py:412, reference zero_points)
 *   tensor_q  int32     [rows, K]            (awq.py:410, reference tensor_q)
 *   qweight   int32     [rows, ceil(K*bits/32)]  packed: element k of a row sits in word
 *             k/(32/bits), bits [bits*(k%(32/bits)), +bits), value (q - qmin) & (2^bits-1)
 *   qzeros    int32     [rows, ceil(G*bits/32)]  same packing of the zero points
 * NaN groups/elements follow the reference: int32 outputs are INT32_MIN (x86 cvtt), packed
 * fields hold (INT32_MIN - qmin) & mask, and NaN scales carry the reference's own bits
 * (awq.py:192-205 -> 327/352 -> 411 on x86 torch CPU; pinned by tests/golden/golden_nan.*):
 *   bf16 input 0x7E00; fp16 input 0x7FFF (small-tensor path: 0xFE00 asymmetric, 0x7E00
 *   symmetric); fp32 / fp64 input 0xFFFF when the group holds a NaN, 0xFE00 when the NaN is
 *   inf - inf (an asymmetric group of all +inf or all -inf); a one-element group keeps its
 *   element's NaN (sign — set when symmetric — and top 10 mantissa bits, quiet bit set).
 */
#ifndef AWQ_HIP_H
#define AWQ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AWQ_HIP_ABI_VERSION 17

/* dtype codes of the input weights (torch dtypes the reference accepts, awq.py:397);
 * the integer codes only in awq_apply_params_ex (integer tensors such as quantize()'s int32
 * tensor_q, and integer ops): I32 .. U8 as tensor and op dtypes, BOOL / U16 / U32 / U64 as
 * tensor dtypes only (ABI 17) */
enum { AWQ_DTYPE_BF16 = 0, AWQ_DTYPE_F16 = 1, AWQ_DTYPE_F32 = 2, AWQ_DTYPE_F64 = 3, AWQ_DTYPE_I32 = 4,
       AWQ_DTYPE_I64 = 5, AWQ_DTYPE_I16 = 6, AWQ_DTYPE_I8 = 7, AWQ_DTYPE_U8 = 8, AWQ_DTYPE_BOOL = 9,
       AWQ_DTYPE_U16 = 10, AWQ_DTYPE_U32 = 11, AWQ_DTYPE_U64 = 12 };

/* status codes */
enum { AWQ_OK = 0, AWQ_EINVAL = 1, AWQ_EUNSUPPORTED = 2, AWQ_EHIP = 3, AWQ_ENODEV = 4 };

/* One tensor of a ragged (multi-tensor) launch.  Same meaning as the awq_quantize_groups
 * arguments.  tile_begin / tile_count are filled by awq_plan_ragged. */
typedef struct awq_tensor_desc {
    const void* w;
    int64_t rows;
    int64_t K;
    int32_t* qweight;
    int32_t* qzeros;
    uint16_t* scales;
    int32_t* tensor_q;
    int32_t* zeros;
    int64_t tile_begin;
    int64_t tile_count;
} awq_tensor_desc;

/* ABI version (AWQ_HIP_ABI_VERSION). */
int awq_abi_version(void);

/* Message of the last failing call on this thread ("" if none). */
const char* awq_last_error(void);

/* AWQ_OK if the current HIP device is a gfx950 (MI355X), AWQ_ENODEV otherwise.
 * Host-only query; writes the device's gcnArchName into arch (if arch != NULL, len > 0). */
int awq_device_check(char* arch, int len);

/* Quantize one [rows, K] tensor (replaces awq.py:286-374 incl. the small-tensor
 * path awq.py:130-171, which a caller expresses as group_size = K).
 * bits in {4, 8}; symmetric selects qmin/qmax per awq.py:114-128.  Kernels, all with the
 * same results:
 *   bf16 / fp16 / fp32, group_size in {32, 64, 128, 256}, K % group_size == 0 or K % 8 == 0
 *     (padded rows, awq.py:337-339): the streaming kernel;
 *   bf16 / fp16 with any other group_size <= 512 (fp32: <= 256), or any K: the row-segment
 *     kernel (packed outputs written directly);
 *   everything else (fp64, larger groups): the generic kernel (one wave per span of groups
 *     sharing a qzeros word; packed outputs written directly too, since round 2).
 * tensor_q / zeros are optional outputs on every path. */
int awq_quantize_groups(const void* w, int dtype, int64_t rows, int64_t K, int32_t group_size,
                        int bits, int symmetric, int32_t* qweight, int32_t* qzeros,
                        uint16_t* scales, int32_t* tensor_q, int32_t* zeros, void* stream);

/* flags of the _ex entry points: the call is the small-tensor path (awq.py:297-300 ->
 * _calculate_scale_zp awq.py:130-171, numel < group_size, expressed as group_size = K): its
 * input-dtype scales reach fp16 directly (awq.py:411) instead of through the fp32 [R, G]
 * buffer of awq.py:327 — only the bits of NaN scales differ (fp16 input, see above). */
#define AWQ_Q_SMALL_TENSOR 1

/* awq_quantize_groups with flags (0 = awq_quantize_groups). */
int awq_quantize_groups_ex(const void* w, int dtype, int64_t rows, int64_t K, int32_t group_size,
                           int bits, int symmetric, int flags, int32_t* qweight, int32_t* qzeros,
                           uint16_t* scales, int32_t* tensor_q, int32_t* zeros, void* stream);

/* Opt-in per-group clip search (scale_method="search"; no reference counterpart: the
 * reference stores scale_method but never uses it, awq.py:66,111-112 — SURVEY.md §8a).
 * Same inputs/outputs as awq_quantize_groups.  For every group the min/max (after the
 * symmetric abs-max, awq.py:196-199) are shrunk by alpha_i = (n_grid - i) / n_grid,
 * i = 0 .. n_candidates-1, each candidate's scale/zero point taken exactly as RTN
 * (awq.py:202-211), and the candidate with the smallest sum of squared errors between
 * the group and its dequantization (awq.py:459-539 arithmetic) is kept; ties and NaN/inf
 * groups keep i = 0, i.e. the RTN result bit-exactly.  1 <= n_candidates <= n_grid.
 * The squared error is summed in fp32 (fp64 for fp64 input) in one canonical order, so
 * every kernel gets the same bits: chunk c = the group's elements 8c .. 8c+7 summed in
 * order, then a pairwise tree over 64 chunk slots, adjacent pairs first (empty slots = 0):
 * group_size <= 512.
 * tensor_q / zeros are optional outputs (no staging buffers needed). */
int awq_quantize_search(const void* w, int dtype, int64_t rows, int64_t K, int32_t group_size, int bits,
                        int symmetric, int n_grid, int n_candidates, int32_t* qweight, int32_t* qzeros,
                        uint16_t* scales, int32_t* tensor_q, int32_t* zeros, void* stream);
/* awq_quantize_search with flags (AWQ_Q_SMALL_TENSOR). */
int awq_quantize_search_ex(const void* w, int dtype, int64_t rows, int64_t K, int32_t group_size, int bits,
                           int symmetric, int flags, int n_grid, int n_candidates, int32_t* qweight,
                           int32_t* qzeros, uint16_t* scales, int32_t* tensor_q, int32_t* zeros, void* stream);

/* The reference's per-group scale and zero point (_compute_scale_zp_for_group, awq.py:173-213)
 * in the input dtype's own arithmetic, as exact doubles [rows, G] (bf16 / fp16 / fp32 / fp64
 * values; NaN groups give NaN).  What _quantize_per_group stores in its fp32 scale / zero
 * tensors (awq.py:327-328, 352-353) is these values rounded to fp32; the small-tensor path
 * (awq.py:130-171) is group_size = K.  Either output may be NULL. */
int awq_group_params(const void* w, int dtype, int64_t rows, int64_t K, int64_t group_size, int bits,
                     int symmetric, double* scales, double* zeros, void* stream);

/* (ABI 17) awq_group_params with flags.  AWQ_GP_TORCH_GPU: the same lines as torch's GPU kernels
 * evaluate them (the reference quantizer with device="cuda"): the scale's division by the Python
 * int qmax - qmin is a product with the reciprocal RN(1 / (qmax - qmin)) in the op's compute
 * type (ATen's GPU division by a CPU scalar), and a zero point clamped from -0 is +0 (the GPU
 * clamp's IEEE maximum).  flags = 0: awq_group_params (torch's CPU semantics). */
#define AWQ_GP_TORCH_GPU 1
int awq_group_params_ex(const void* w, int dtype, int64_t rows, int64_t K, int64_t group_size, int bits,
                        int symmetric, int flags, double* scales, double* zeros, void* stream);

/* Elementwise with caller-given parameters per group (scales / zeros double [rows, G], used
 * in the op's compute type — fp32, fp64 for fp64 inputs — unrounded to the input dtype, as
 * torch's CPU kernels use a 0-d operand; group_size 1 = one parameter per element), result
 * in the input dtype (out [rows, K]):
 *   mode 0: clamp(round(RN(RN(x / s) + z)), qmin, qmax)   (_quantize_tensor, awq.py:215-250;
 *           NaN stays NaN)
 *   mode 1: RN(RN(x - z) * s)                             (_dequantize_tensor, awq.py:252-284) */
int awq_apply_params(const void* x, int dtype, int64_t rows, int64_t K, int64_t group_size, const double* scales,
                     const double* zeros, int qmin, int qmax, int mode, void* out, void* stream);

/* awq_apply_params_ex flags: the scale / zero point is a one-element operand of the
 * reference's expression (any shape of numel 1) evaluated by torch's CPU kernels (a
 * reference quantizer with device="cpu"; on CUDA a one-element device tensor is converted to
 * the op dtype like any other operand: leave the flag off) */
#define AWQ_APPLY_SCALE_ONE_ELEMENT 1
#define AWQ_APPLY_ZERO_ONE_ELEMENT 2
/* (ABI 17) the scales / zeros array holds int64 values, not doubles (an integer or bool
 * parameter, exact beyond 2^53); _UNSIGNED: those 64-bit words are uint64 values */
#define AWQ_APPLY_SCALE_INT 4
#define AWQ_APPLY_ZERO_INT 8
#define AWQ_APPLY_SCALE_UNSIGNED 16
#define AWQ_APPLY_ZERO_UNSIGNED 32
/* (ABI 17) mode 0's clamp as torch's GPU kernels evaluate it: clamp(-0, 0, qmax) = +0 (IEEE
 * maximum); without it the -0 stays, as torch's CPU clamp keeps an operand equal to the bound.
 * Together with the ONE_ELEMENT flags left off: the reference quantizer with device="cuda". */
#define AWQ_APPLY_IEEE_CLAMP 64

/* The same two ops with torch's type promotion (ABI 15; replaces awq.py:245 and awq.py:282 for
 * parameters of any dtype, e.g. bf16 weights with fp32 per-channel scales, or quantize()'s
 * int32 tensor_q dequantized with fp16 scales):
 *   mode 0: a = x / s in op1_dtype; t = a + z in op2_dtype; round, clamp(qmin, qmax)
 *   mode 1: a = x - z in op1_dtype; t = a * s in op2_dtype
 * op1_dtype / op2_dtype are torch's result dtypes of the two ops (the caller's promotion);
 * out [rows, K] is op2_dtype.  x_dtype may be any integer code too (int64 / int32 / int16 /
 * int8 / uint8 / bool / uint16 / uint32 / uint64 tensors: the reference evaluates awq.py:245 and
 * :282 for any tensor dtype), the op dtypes I32 .. U8 (mode 1 only; integer ops wrap at their
 * width like torch's integer kernels).  Each op: operands converted to its dtype (c10::convert:
 * a float to bf16 / fp16 through fp32; an integer to a float dtype as RN_f32 of the exact
 * integer, then RN to bf16 / fp16, to fp64 directly; to an integer dtype by truncation), fp32
 * math for bf16 / fp16 / fp32 (fp64 for fp64), result rounded to the dtype — except that a
 * parameter flagged AWQ_APPLY_*_ONE_ELEMENT enters a bf16 / fp16 op at its own value in fp32
 * (ATen's reduced-float CPU kernels read a one-element operand's original value).  scales /
 * zeros: the parameters' exact values as doubles (or int64 / uint64 words, AWQ_APPLY_*_INT),
 * [rows, G] as in awq_apply_params (group_size 1 = one per element).
 * awq_apply_params(x, D, ...) = awq_apply_params_ex(x, D, ..., D, D, both flags, ...). */
int awq_apply_params_ex(const void* x, int x_dtype, int64_t rows, int64_t K, int64_t group_size,
                        const double* scales, const double* zeros, int qmin, int qmax, int mode, int op1_dtype,
                        int op2_dtype, int flags, void* out, void* stream);

/* 1 if awq_quantize_groups writes qweight / qzeros for this dtype / shape without the int32
 * tensor_q / zeros staging buffers.  Since round 2 every kernel does (the generic kernel packs
 * per span of groups), so this is 1 for every supported dtype; kept for ABI compatibility. */
int awq_packs_directly(int dtype, int64_t rows, int64_t K, int64_t group_size);

/* True (1) if a tensor of this dtype/shape is eligible for awq_quantize_ragged. */
int awq_ragged_eligible(int dtype, int64_t rows, int64_t K, int64_t group_size);

/* HOST helper: fills descs[i].tile_begin / tile_count (host array) for a ragged launch
 * and returns the total tile count (< 0 on error).  All tensors must be eligible for this
 * group_size (32, 64, 128 or 256; a tile is 2048 elements = 2048 / group_size groups). */
int64_t awq_plan_ragged(awq_tensor_desc* descs_host, int n, int bits, int64_t group_size);

/* Tiles per entry of the ragged launch's tensor table (awq_plan_block_tensor); the kernel's
 * workgroup size is the library's own business (one 64-lane wave per tile). */
#define AWQ_BLOCK_TILES 8

/* HOST helper: the ragged launch's tensor table, one 64-B entry per AWQ_BLOCK_TILES tiles
 * (opaque to the caller: 16 int32 each; ceil(total_tiles / 128) * 16 entries): the input
 * pointer, first tile and shape of the tensor holding the entry's first tile (so a wave
 * issues its loads after one scalar load) and its descriptor index, with bit 31 set when
 * the entry's tiles span more than one tensor (a wave then steps forward from there to its
 * own).  An entry's tiles are the 8 tiles of one XCD in a 64-tile window (t0 + 8 j), so
 * each 128-B line of the table is read by one XCD.  Returns the number of int32
 * written (< 0 on error: len too small, or block_tensor_host not 16-B aligned);
 * block_tensor_host = NULL with len = 0 returns the length needed without writing.
 * descs_host as planned by awq_plan_ragged (the pointers are the device pointers the
 * launch will read). */
int64_t awq_plan_block_tensor(const awq_tensor_desc* descs_host, int n, int64_t total_tiles,
                              int32_t* block_tensor_host, int64_t len);

/* flags of awq_quantize_ragged: some tensor has K % group_size != 0 (padded rows: the
 * kernel instance with the row-tile path; the others are built without it) */
#define AWQ_RAGGED_PADDED 1

/* HOST helper: the awq_quantize_ragged flags a descriptor array needs. */
int awq_ragged_flags(const awq_tensor_desc* descs_host, int n, int64_t group_size);

/* Quantize n eligible tensors of one dtype (AWQ_DTYPE_BF16, _F16 or _F32) in ONE
 * launch (replaces the CLI's per-tensor loop, main.py:353-392).  descs_device: device copy
 * of the array planned by awq_plan_ragged with the same bits and group_size (the caller
 * uploads it; reusable across calls).  block_tensor_device: optional device copy of the
 * awq_plan_block_tensor table (NULL: each wave searches the descriptors). */
int awq_quantize_ragged(const awq_tensor_desc* descs_device, int n, int64_t total_tiles,
                        const int32_t* block_tensor_device, int dtype, int bits, int symmetric, int64_t group_size,
                        int flags, void* stream);

/* awq_quantize_ragged with the opt-in clip search of awq_quantize_search (round 5): the same
 * bits as awq_quantize_search on every tensor of the batch, one launch for a model's tensor
 * set.  1 <= n_candidates <= n_grid (n_candidates = 1: plain RTN, awq_quantize_ragged). */
int awq_quantize_ragged_search(const awq_tensor_desc* descs_device, int n, int64_t total_tiles,
                               const int32_t* block_tensor_device, int dtype, int bits, int symmetric,
                               int64_t group_size, int flags, int n_grid, int n_candidates, void* stream);

/* AutoAWQ "GEMM" layout (the reference has no packed format): from
 * this library's row-major packed 4-bit results of an [N = out_features, K = in_features]
 * weight (qweight [N, K/8], qzeros [N, ceil(G/8)], scales fp16 [N, G], G = K / group_size)
 * to qweight_t int32 [K, N/8], qzeros_t int32 [G, N/8], scales_t fp16 [G, N], packed along
 * N with AWQ_ORDER {0,2,4,6,1,3,5,7} (nibble i of word c = column 8c + AWQ_ORDER[i]).
 * bits must be 4; N % 8 == 0; K % group_size == 0. */
int awq_export_autoawq_gemm(const int32_t* qweight, const int32_t* qzeros, const uint16_t* scales, int64_t N,
                            int64_t K, int64_t group_size, int bits, int32_t* qweight_t, int32_t* qzeros_t,
                            uint16_t* scales_t, void* stream);

/* The exact inverse of awq_export_autoawq_gemm (additive to ABI 17): from qweight_t int32
 * [K, N/8], qzeros_t int32 [G, N/8], scales_t fp16 [G, N] (nibble i of word c = column
 * 8c + AWQ_ORDER[i]) back to this library's row-major qweight [N, K/8], qzeros [N, ceil(G/8)]
 * (the unused high fields of a row's last word, G % 8 != 0, are 0: import(export(p)) == p word
 * for word) and scales [N, G].  Caller-owned device memory on the caller's stream; no
 * allocation, no sync.  Any output may be NULL (its input is then not looked at); at least one
 * must not be.  Pointers need 4-B (scales: 2-B) alignment; 16-B aligned ones take the wide
 * accesses.  bits must be 4; N % 8 == 0; K % group_size == 0; the export's size limit. */
int awq_import_autoawq_gemm(const int32_t* qweight_t, const int32_t* qzeros_t, const uint16_t* scales_t, int64_t N,
                            int64_t K, int64_t group_size, int bits, int32_t* qweight, int32_t* qzeros,
                            uint16_t* scales, void* stream);

/* ---- AutoGPTQ layout, 4 bits, desc_act = false (additive to ABI 17): from this
 * library's row-major packed 4-bit results of an [N = out_features, K = in_features] weight
 * (qweight [N, K/8], qzeros [N, ceil(G/8)], scales fp16 [N, G], G = K / group_size) to
 *   qweight_t int32 [K/8, N]   nibble i of word (r, n) = u[n, 8r + i]   (sequential, no interleave)
 *   qzeros_t  int32 [G, N/8]   nibble i of word (g, c) = zs[g, 8c + i]  (sequential)
 *   scales_t  fp16  [G, N]     the scale bits, transposed
 *   g_idx     int32 [K]        k / group_size
 * A packed field of this library is q - qmin: u = q and z' = z when asymmetric, u = q + 8 and
 * z' = 8 when symmetric ((u - z') s = q s exactly), so u and z' are the stored fields in both
 * modes and `symmetric` (0 or 1) changes no bit of the transform.  zero_offset selects the stored
 * zero: 1 (checkpoint_format "gptq", v1) zs = (z' - 1) & 15; 0 ("gptq_v2") zs = z'.
 * Checked in this order, nothing launched on a failure: a negative N or K: AWQ_EINVAL; bits != 4:
 * AWQ_EUNSUPPORTED; group_size <= 0, N % 8, K % 8 or K % group_size != 0: AWQ_EINVAL; zero_offset
 * or symmetric outside {0, 1}: AWQ_EINVAL; N == 0 or K == 0: AWQ_OK, no pointer is looked at; N or
 * K above 65535 * 256 (the AutoAWQ export's limit) or N K > 2^42: AWQ_EUNSUPPORTED; no output:
 * AWQ_EINVAL; an output whose input is NULL: AWQ_EINVAL.  Any output may be NULL (its input is
 * then not read); at least one must not be.  Caller-owned device memory on the caller's stream;
 * no allocation, no sync.  Pointers need 4-B (scales: 2-B) alignment; 16-B aligned ones with
 * K % 32 == 0 (scales: G % 8 == 0) take 16-B accesses, which give the same bits. */
int awq_export_gptq(const int32_t* qweight, const int32_t* qzeros, const uint16_t* scales, int64_t N, int64_t K,
                    int64_t group_size, int bits, int symmetric, int zero_offset, int32_t* qweight_t,
                    int32_t* qzeros_t, uint16_t* scales_t, int32_t* g_idx, void* stream);

/* The exact inverse of awq_export_gptq with the same zero_offset: import(export(p)) == p word for
 * word; z' = (zs + zero_offset) & 15, and the unused high fields of a row's last qzeros word
 * (G % 8 != 0) are 0.  The same checks in the same order.  Nothing on the device is refused: a
 * symmetric checkpoint whose stored zero is not 8 imports as it is stored (the Python reader
 * reports it); g_idx is not an input (act-order is not supported). */
int awq_import_gptq(const int32_t* qweight_t, const int32_t* qzeros_t, const uint16_t* scales_t, int64_t N, int64_t K,
                    int64_t group_size, int bits, int symmetric, int zero_offset, int32_t* qweight, int32_t* qzeros,
                    uint16_t* scales, void* stream);

/* ---- GPTQ error-compensated rounding, one block of input columns (additive to ABI 17; no reference
 * counterpart) ----
 * Rounds columns [col_begin, col_begin + n_cols) of the fp32 working weights work [N, K] one column
 * at a time and takes each column's error off the block's later columns through u, the fp32 [K, K]
 * row-major upper-triangular factor with H^-1 = u^T u (H: the damped Hessian X^T X of the layer's
 * input).  The caller then updates the columns right of the block (work[:, c1:] -= err u[c0:c1, c1:])
 * and calls the next block; qweight / qzeros / scales are this library's packed result of the WHOLE
 * [N, K] tensor (the layouts at the top of this file), of which a call writes only its block's
 * qweight words, zero FIELDS (a read-modify-write of the word: the caller zero-fills qzeros once, so
 * the pad fields of a row's last word are 0) and fp16 scales.
 * Per row, for i = 0 .. n_cols - 1, c = col_begin + i, every operation a single fp32 operation:
 *   at a group's first column: (scale, zero) = this library's fp32 rule (awq_quantize_groups on fp32
 *     input) on the group's group_size working values as they stand now; the scale's fp16 bits are
 *     stored as that entry stores them, and s = (float)fp16(scale) is what the steps below use;
 *   quo = w[i] / s (IEEE), q = clamp(rint(quo) + zero, qmin, qmax), dq = (q - zero) s; a NaN
 *     rint(quo) + zero stores the NaN field (INT32_MIN - qmin) & mask and dq = NaN;
 *   e = (w[i] - dq) / u[c][c] (IEEE), e = 0 when s, dq or quo is not finite (a constant, NaN or inf
 *     group propagates nothing); err[row, i] = e;
 *   for j > i in the block: w[j] = RN(w[j] - RN(e u[c][col_begin + j])), no contraction.
 * work's block columns hold the final w (a rounded column keeps the value it was rounded from).
 * bits 4 / 8, symmetric 0 / 1, group_size 32 / 64 / 128.  Checked in this order, nothing launched on
 * a failure: a negative N, K, col_begin or n_cols (AWQ_EINVAL); bits (AWQ_EUNSUPPORTED); symmetric
 * outside {0, 1} (AWQ_EINVAL); group_size (AWQ_EUNSUPPORTED); K % group_size; n_cols > 128 or
 * n_cols % group_size; col_begin % group_size, col_begin % 8 or col_begin + n_cols > K (AWQ_EINVAL);
 * N, K or n_cols of 0: AWQ_OK, no pointer is looked at; N or K >= 2^31 (AWQ_EUNSUPPORTED); a NULL
 * pointer; work, u or err not 16-B aligned, qweight / qzeros not 4-B, scales not 2-B (AWQ_EINVAL).
 * err fp32 [N, n_cols].  One lane per row, one workgroup per 64 rows, the grid is not capped.
 * Caller-owned device memory on the caller's stream; no allocation, no sync. */
int awq_gptq_round_block(float* work, int64_t N, int64_t K, int64_t group_size, int bits, int symmetric,
                         const float* u, int64_t col_begin, int64_t n_cols, float* err, int32_t* qweight,
                         int32_t* qzeros, uint16_t* scales, void* stream);

/* Measurement helper: copy `bytes` (multiple of 16, 16-B aligned buffers) with the
 * quantizer's memory structure (one wave per 4 KiB, 16-B nt loads/stores); bench.py
 * quotes the kernel against this copy's rate. */
int awq_stream_copy(const void* src, void* dst, int64_t bytes, void* stream);

/* Measurement helper: the quantizer's read-dominant memory structure without its
 * arithmetic — reads `bytes` (multiple of 4096, 16-B aligned) in 4 KiB waves and writes
 * bytes / 4 to dst (one 16-B store per lane per 4 KiB).  bench.py quotes the kernel
 * against this stream's (read + write) rate. */
int awq_stream_ceiling(const void* src, void* dst, int64_t bytes, void* stream);

/* Measurement helper (ABI 17): awq_dequantize_packed's memory structure for 4-bit outputs without
 * its arithmetic — reads out_bytes / 8 of `words` (4-B aligned; 4-B nt loads, a lane pair per
 * dword) and writes out_bytes (16-B aligned, multiple of 16) as 16-B nt stores, 1 KiB per wave
 * instruction: the 1 : 8 read : write stream the dequantize kernel is quoted against
 * (scripts/dq_ceiling_bench.py). */
int awq_dequant_ceiling(const void* words, void* out, int64_t out_bytes, void* stream);

/* Reference dequantize (awq.py:459-539): out fp32 [rows, K] =
 * fp16( fp16(tensor_q - zeros) * scales ) per element.  A NaN result widens its fp16 bits,
 * except in the last n % 8 elements of a group of n = min(group_size, K - g group_size)
 * elements, where it is 0x7FFFFFFF (the reference's fp16 -> fp32 copy, awq.py:527/531). */
int awq_dequantize(const int32_t* tensor_q, const uint16_t* scales, const int32_t* zeros,
                   int64_t rows, int64_t K, int64_t group_size, float* out, void* stream);

/* Same from the packed outputs (qweight/qzeros/scales) of the same bits/symmetric. */
int awq_dequantize_packed(const int32_t* qweight, const int32_t* qzeros, const uint16_t* scales,
                          int64_t rows, int64_t K, int64_t group_size, int bits, int symmetric,
                          float* out, void* stream);

/* Pack int32 values [rows, n] into [rows, ceil(n*bits/32)] words ((v - qmin) & mask). */
int awq_pack_rows(const int32_t* v, int64_t rows, int64_t n, int bits, int qmin, int32_t* packed,
                  void* stream);

/* ---- Quantization-error report (additive to ABI 17; no reference counterpart beyond the
 * per-tensor torch.abs(tensor - dequantized).mean() its test_quantization.py:155-160 prints) ----
 * What the packed result (qweight / qzeros / scales above, any scale method) costs against the
 * original weights w [rows, K] (bf16 / fp16 / fp32; fp64 and group_size > 512: AWQ_EUNSUPPORTED),
 * in one pass over w and qweight, without materialising the dequantized tensor.  Per element k of
 * group g:  dq = fp32(fp16(fp16(q - z) * s)) (awq_dequantize_packed's arithmetic),
 *   d = RN_f32(fp32(w) - dq), a = |d|, e = RN_f32(d d), p = RN_f32(fp32(w) fp32(w)), no contraction;
 *   an element whose d, e or p is NaN / +-inf adds nothing to the sums or the max and counts 1.
 * Level 1, per group, fp32: the sums of a, e, p over the group's finite elements in
 *   awq_quantize_search's canonical order (8-element chunks in sequence from +0, then the pairwise
 *   tree over 64 chunk slots, adjacent pairs first), the max of a (+0 if none), the count (int32).
 * Level 2, per tensor, fp64: each of the three sums over the flat groups r G + g in
 *   awq_act_search_select's four ascending levels (64-group sub-blocks, 1024-group blocks,
 *   32-block super-blocks, the super-blocks); the max of the maxes; the sum of the counts.
 * Kernels, all with the same bits: group_size 32 / 64 / 128 / 256 with K % group_size == 0 and 16-B
 * aligned w / qweight: the streaming kernel (one wave per 2048 elements); everything else
 * (any K, tail groups, element-aligned pointers): one wave per group.  rows * G < 2^31. */

/* bytes of the fp64 workspace awq_quant_error needs (< 0: unsupported shape) */
int64_t awq_quant_error_work_bytes(int64_t rows, int64_t K, int64_t group_size);
/* group_stats fp32 [4, rows*G]: sum|d|, sum d^2, sum w^2, max|d| per group; group_nonfinite int32 [rows*G];
 * totals fp64 [5] (device): the three level-2 sums, max|d|, non-finite count.  group_stats / group_nonfinite
 * are caller buffers and are always written (they are level 1); totals may be NULL (work is then unused). */
int awq_quant_error(const void* w, int dtype, int64_t rows, int64_t K, int64_t group_size, int bits, int symmetric,
                    const int32_t* qweight, const int32_t* qzeros, const uint16_t* scales, float* group_stats,
                    int32_t* group_nonfinite, double* work, double* totals, void* stream);

/* ---- Output-space error on token samples (additive to ABI 17; beyond the reference: it replaces
 * no reference function) ----
 * What the packed result (qweight / qzeros / scales above, row-major) costs at a linear's OUTPUT on
 * calibration samples x [T, K] (dtype D of w, row stride x_row_stride >= K elements), against the
 * original weights w [N, K] (D = bf16 / fp16 / fp32; fp64: AWQ_EUNSUPPORTED).  Per element:
 *   dq = fp32(fp16(fp16(q - z) * s))                         (awq_quant_error's, awq_dequantize_packed's)
 *   w^ = dq if col_scale is NULL, else RN_f32(dq / col_scale[k])   (IEEE division; col_scale fp32 [K]:
 *        the input scale a result of W * diag(s) was quantized with, so w^ is in w's own domain)
 *   d  = RN_f32(w^ - fp32(w)), no contraction.
 * E[n, t] = sum_k d[n, k] x[t, k], R[n, t] = sum_k w[n, k] x[t, k];
 * err_sq[n] = sum_t E^2, ref_sq[n] = sum_t R^2 (ref_sq may be NULL); err [N, T], when not NULL,
 * receives E itself.  Nothing is masked: a non-finite d, w or x makes the sums that contain it
 * non-finite, as IEEE arithmetic gives.
 * Accuracy: the order of the sum over k is the implementation's (the matrix core's), so the contract
 * is a bound: |E - E_exact| <= eps_K * sum_k |d| |x| with eps_K = 2^-17 + K 2^-22 (d enters as the two
 * bf16 terms d_hi = RN_bf16(d), d_lo = RN_bf16(d - d_hi): within 2^-17 |d| of d; the products are exact,
 * 2 K of them accumulate in fp32), the same for R with |w| for |d|; the sum over t adds at most
 * (T + 1) 2^-24 relative on the computed E^2.  No floating-point atomics: every (128-token tile, row)
 * writes one fp32 partial to `work` and a second kernel adds the tiles in ascending order, so the
 * results are the same bits from run to run.
 * Kernels: bf16 with group_size 32 / 64 / 128 / 256, 16-B aligned w / x / qweight, x_row_stride % 8
 * == 0 (and K, x_row_stride < 2^22): v_mfma_f32_32x32x16_bf16 on the hi / lo split; everything else:
 * v_mfma_f32_16x16x4_f32 on f32 operands.
 * Refused: bits other than 4 / 8, x_row_stride < K (AWQ_EINVAL); a group_size that is not a power of
 * two in [8, 512], K % group_size != 0, N K, N T or T x_row_stride above 2^60 (AWQ_EUNSUPPORTED).
 * N, K or T of 0: AWQ_OK, nothing is read or written. */

/* bytes of the workspace awq_output_error needs: fp32 [2][ceil(T / 128)][N] (0 for an empty or
 * refused shape) */
int64_t awq_output_error_work_bytes(int64_t N, int64_t T);
int awq_output_error(const void* w, int dtype, int64_t N, int64_t K, int64_t group_size, int bits, int symmetric,
                     const int32_t* qweight, const int32_t* qzeros, const uint16_t* scales,
                     const float* col_scale,            /* [K] or NULL (= 1) */
                     const void* x, int64_t T, int64_t x_row_stride,   /* samples [T, K] of `dtype`, stride in elements */
                     void* work, float* err_sq,         /* [N] */
                     float* ref_sq,                     /* [N] or NULL */
                     float* err,                        /* [N, T] or NULL */
                     void* stream);

/* ---- Host streaming pipeline ----------------------------------
 * Replaces the CLI's read -> quantize -> collect loop (reference main.py:216-392, which
 * loads every file whole and then quantizes tensor by tensor): tensors are pread from their
 * safetensors files straight into pinned staging slots by native reader threads, copied to
 * HBM on an H2D stream, quantized on the compute stream by one ragged launch per dtype and
 * batch (awq_quantize_ragged; shapes it does not take: awq_quantize_groups_ex per tensor),
 * and their outputs copied back on a D2H stream — read, H2D, kernels and D2H of neighbouring
 * batches overlap, with no per-tensor work in the host language.  A 2-D tensor larger than
 * what is left of a slot is split by rows (rows quantize independently, awq.py:332-368), so
 * slots stay small (pipeline fill) whatever the largest tensor.
 *
 * Caller-owned memory: staging slots (pinned host + device), per-slot descriptor tables
 * (pinned host + device, awq_stream_table_bytes each), every item's device outputs and, when
 * its results are wanted on the host, a pinned host range of the same size.  Streams (ABI
 * 14): a stream left NULL in the config is created by the pipeline (non-blocking) and
 * destroyed by awq_stream_end, on its submitter thread while the readers fill the first
 * slots; a non-NULL stream is the caller's.  The submitter first joins the device's
 * first-use warm-up (awq_runtime_warmup below), or runs it if nobody started it. */

/* HIP's first-use costs of a process on a device — its first hardware queue (~85 ms on
 * MI355X), first large copy (~7 ms) and the code object of the quantize kernels (~9 ms) —
 * paid on a native thread of its own: three non-blocking streams (kept for the device's
 * first pipeline, whose NULL config streams they become), one 8 MiB H2D, copy kernel and
 * D2H (buffers freed after).  Returns at once; a later call for the same device does nothing.
 * A CLI starts it as soon as it knows its device, so the costs overlap its host-side setup
 * (file index, planning, pinned allocations). */
int awq_runtime_warmup(int device);

/* Join the device's warm-up if it was started (else return at once); *seconds (may be NULL)
 * = its duration.  Call it before the process exits if the warm-up may still run. */
int awq_runtime_warmup_wait(int device, double* seconds);

/* (awq_stream_*, continued)
 *
 * Bounded output memory (round 4): the caller may place the items' device outputs and host
 * ranges in two RINGS that later items reuse, with two per-item gates:
 *   dev_gate  = g > 0: the kernels writing this item's outputs first wait (on the compute
 *               stream, no host block) for the D2H of items [0, g) — the earlier items whose
 *               device ranges this item's overlap;
 *   host_gate = g > 0: the D2H into this item's host range waits until the caller has
 *               released items [0, g) (awq_stream_release: it no longer reads their host
 *               results, e.g. once their output files are written).
 * awq_stream_plan gives the batch of every item's first and last piece before the start,
 * so the caller can place the rings; awq_stream_start rejects a dev_gate that would wait
 * for a D2H of the same or a later batch, and a host_gate > the item's index.  A caller
 * that releases only what the items before a batch let it release must size the host ring
 * so that a batch's gate never needs that batch's own items (awq_stream_plan).
 *
 * scale_method="search" (awq_quantize_search) runs through the pipeline too: config
 * search_candidates > 0 makes every piece's launch awq_quantize_search_ex with
 * search_grid / search_candidates (rows are independent, so a row split gives the bits of
 * the whole-tensor call). */
#define AWQ_STREAM_MAX_BATCH_ITEMS 4096

typedef struct awq_stream_item {
    int32_t fd;          /* readable file descriptor (pread) */
    int32_t dtype;       /* AWQ_DTYPE_* of the stored tensor */
    int64_t offset;      /* byte offset of the tensor's data in the file */
    int64_t rows, K;     /* awq.py:306-320: rows = dim 0 (1 for a 1-D tensor), K = the rest */
    int32_t* qweight;    /* device outputs (any may be NULL), as awq_quantize_groups */
    int32_t* qzeros;
    uint16_t* scales;
    int32_t* tensor_q;
    int32_t* zeros;
    void* dev_out;       /* D2H of [dev_out, dev_out + out_bytes) (the item's outputs, laid out */
    void* host_out;      /* by the caller inside that range) into pinned host_out; NULL: none */
    int64_t out_bytes;
    void* dev_out2;      /* a second range (e.g. the fp16 scales, kept in a buffer of their */
    void* host_out2;     /* own dtype), NULL: none */
    int64_t out_bytes2;
    int32_t dev_gate;    /* 0: none; see "Bounded output memory" above */
    int32_t host_gate;   /* 0: none */
} awq_stream_item;

typedef struct awq_stream_config {
    int32_t bits, symmetric, group_size, readers;   /* readers: pread threads (>= 1) */
    int32_t nslots;                                 /* >= 2 */
    int32_t trace_batches;                          /* capacity of `trace`, in batches */
    int32_t search_grid, search_candidates;         /* scale_method="search"; 0 candidates = RTN */
    int64_t slot_bytes;          /* input bytes per staging slot, multiple of 4096 */
    int64_t first_batch_bytes;   /* capacity of the first batch (<= slot_bytes; 0 = slot_bytes) */
    void* host_staging;          /* pinned host, nslots * (awq_stream_table_bytes(slot_bytes) +
                                    slot_bytes): each slot = its batch's descriptor / tensor-table
                                    area, then its input; one H2D carries both */
    void* dev_staging;           /* device, the same size */
    void* compute_stream;        /* NULL: the pipeline's own (see above) */
    void* h2d_stream;
    void* d2h_stream;
    double* trace;               /* optional (NULL = off): AWQ_STREAM_TRACE_FIELDS doubles per
                                    batch, seconds from the start, filled by awq_stream_end:
                                    first read began, last read ended, H2D enqueued, kernels
                                    enqueued, D2H enqueued (host clock); H2D done, kernels done,
                                    D2H done (HIP event clock, from an event on the H2D stream,
                                    offset to the host clock at its recording); seconds spent
                                    inside the H2D call and
                                    inside the D2H calls; seconds of the batch's host planning,
                                    of waiting for the slot's previous kernels, of the ragged
                                    launches and of the per-tensor launches;
                                    batches past trace_batches are not traced. */
} awq_stream_config;

#define AWQ_STREAM_TRACE_FIELDS 14

typedef struct awq_stream_stats {
    int64_t batches, pieces, bytes_read;
    double wall_s;               /* start -> last batch's outputs ready */
    double read_busy_s;          /* summed over reader threads */
    double wait_read_s;          /* submitter waiting for a batch's reads */
    double wait_slot_s;          /* submitter waiting for a slot's previous kernels */
    double wait_release_s;       /* submitter waiting for host-ring releases (host_gate) */
    double prepare_s;            /* submitter's device preparation (streams, first-use warm-up) */
} awq_stream_stats;

/* Per-slot descriptor / tensor-table bytes (descriptors + tensor tables of up to
 * AWQ_STREAM_MAX_BATCH_ITEMS pieces): the head of every staging slot; a multiple of 4096. */
int64_t awq_stream_table_bytes(int64_t slot_bytes);

/* HOST only: the batches awq_stream_start would plan for these items and this config
 * (same slot_bytes / first_batch_bytes), without starting anything: first_batch[i] /
 * last_batch[i] = the batch of item i's first / last piece (an item without elements:
 * the batch that completes it, both).  Returns the number of batches (< 0: error). */
int64_t awq_stream_plan(const awq_stream_item* items, int n, const awq_stream_config* cfg, int32_t* first_batch,
                        int32_t* last_batch);

/* Plan the batches and start the pipeline on its own native threads; returns at once.
 * *handle receives the pipeline (awq_stream_end frees it).  Items are processed in order. */
int awq_stream_start(const awq_stream_item* items, int n, const awq_stream_config* cfg, void** handle);

/* The caller no longer reads the host results of items [0, items) (monotone: a smaller
 * count than an earlier call is ignored); wakes a D2H waiting on a host_gate. */
int awq_stream_release(void* handle, int32_t items);

/* Number of batches of a started pipeline. */
int64_t awq_stream_batches(void* handle);

/* Block until batch b's outputs are ready (on the host for items with host_out, on the
 * device otherwise); [*first_item, *end_item) = the items whose last piece is in batch b.
 * Returns the pipeline's first error (its message in awq_last_error), if any. */
int awq_stream_wait(void* handle, int64_t batch, int32_t* first_item, int32_t* end_item);

/* Wait for the whole pipeline, join its threads, release the handle; stats may be NULL.
 * Returns the first error of the pipeline.  Batches not yet copied back when it is called
 * (the caller stopped early) are cancelled rather than copied into host ranges the caller
 * may still be reading. */
int awq_stream_end(void* handle, awq_stream_stats* stats);

/* ---- Activation-aware per-input-channel scale search (scale_method="awq") ----------
 * Not in the reference (it stores scale_method, awq.py:66, and collects no activations;
 * parity unpinned).  AutoAWQ's published search (third-party,
 * not vendored in the reference) restated with a per-element loss, for one "layer group"
 * of n >= 1 linears W_j [R_j, K] that read the same input x [tokens, K]:
 *
 *   x_mean[k] = fp32(sum_t |x[t,k]| / T),  x_sq[k] = fp32(sum_t x[t,k]^2 / T)
 *       (awq_act_stats; sums in fp64: t ascending inside 32-token sub-blocks, the
 *        sub-blocks ascending inside 256-token blocks, then the blocks ascending)
 *   w_mean[k] = fp32(sum_{j,r} fp32(|W_j[r,k]| / fp32(gmax_j[r, k/gs] + 1e-6f)) / sum_j R_j)
 *       (duo scaling only; gmax = max |W| of the group; same fp64 block order, the
 *        linears' blocks in list order; awq_weight_colsum per linear + awq_column_mean)
 *   candidate i = 0 .. n_grid-1, r = i / n_grid (fp64):
 *       raw_k = max(awq_pow(x_mean_k, r) [/ (awq_pow(w_mean_k, 1-r) + 1e-4)], 1e-4)
 *       s_i[k] = fp32(raw_k / sqrt(max_k raw * min_k raw)), inf / NaN -> 1
 *       (awq_act_scale_table; fp64, IEEE-rounded / and sqrt)
 *   awq_pow(x, r) (round 5; not libm pow, whose last bit differs between math libraries):
 *       r == 0 -> 1; NaN or x < 0 -> NaN; x == 0 -> 0; x == inf -> inf; else, in IEEE fp64
 *       with explicit fma and no other contraction:
 *       ln x: x = m 2^e, m in [sqrt(2)/2, sqrt(2)) (subnormal x scaled by 2^54 first),
 *             f = (m-1)/(m+1); P = 1/25, P = fma(P, f*f, 1/(2j+1)) for j = 11 .. 1;
 *             ln m = fma(2f * (f*f), P, 2f); ln x = fma(e, LN2_HI, fma(e, LN2_LO, ln m))
 *             (LN2_HI = 0x1.62e42feep-1, LN2_LO = 1.90821492927058770002e-10)
 *       e^y:  k = rint(y * 1.44269504088896338700), t = fma(-k, LN2_LO, fma(-k, LN2_HI, y)),
 *             p = 1, p = fma(p, t / j, 1) for j = 15 .. 1; result p * 2^k (k > 1023:
 *             (p 2^1023) 2^(k-1023); k < -1022: (p 2^(k+600)) 2^-600; y > 709.8 -> inf,
 *             y < -746 -> 0)
 *       x^r = e^(r * ln x) — within 2^-40 of x^r over the fp32 range, and the same bits in
 *       every implementation (oracle_act_scale_table restates it)
 *   per element of every group, in the weight dtype D's per-op rounding:
 *       w' = RN_D(w * s_i[k]); RTN scale/zero of w' (awq.py:173-213); q (awq.py:245-248);
 *       dq = fp16(fp16(q - z) * fp16(scale)) (awq.py:459-539); e = fp32(dq / s_i[k]) - w;
 *       c = x_sq[k] * (e * e)
 *   group loss: each 8-element chunk summed in order, then the pairwise tree over the
 *       group's gs/8 chunks (fp32) -> part[i * part_stride + group]
 *       (awq_act_search_losses, per linear at its offset in one group list)
 *   loss_i = fp64 sum in four ascending levels: groups inside a 64-group sub-block,
 *       sub-blocks inside a 1024-group block, blocks inside a 32-block super-block, then
 *       the super-blocks; best = first minimum (NaN never wins; all NaN -> 0)
 *       (awq_act_search_select)
 *   result: every W_j quantized as W_j * diag(s_best) (awq_apply_input_scale, then
 *       awq_quantize_groups); s_best is returned to be folded into the op producing x
 *       (x / s_best, e.g. the preceding norm's weight).
 * The loss is the diagonal (uncorrelated-channel) form of AutoAWQ's output MSE
 * ||x (W' - W)^T||^2.  Weights: bf16 / fp16 / fp32, 2-D, K % gs == 0, gs a power of two in
 * [8, 512]; weights / table / x_sq 16-B aligned.  Sizes of the caller's workspaces:
 *   awq_act_stats      work    fp64 [2 * ceil(T/256) * K]
 *   awq_weight_colsum  gmax_work fp32 [R * K/gs] (scratch of the two-pass path; gs 32 / 64 /
 *                      128 / 256 with 16-B aligned w take the one-pass kernel and leave it
 *                      untouched); partial fp64 [ceil(R/256) * K] (this linear's slice of the
 *                      group's [sum_j ceil(R_j/256), K] array)
 *   awq_act_search_select work fp64 [n_grid * ceil(part_stride / 1024)]
 *   awq_act_scale_table_ws work fp64 [n_grid * (K + 3 * ceil(K / 256))]
 * n_grid <= AWQ_ACT_MAX_GRID; part_stride <= 6144 * 32 * 1024 groups (201 326 592: the
 * select kernel's super-block sums of one candidate fit its LDS), else hipErrorInvalidValue. */
#define AWQ_ACT_MAX_GRID 256

int awq_act_stats(const void* x, int dtype, int64_t tokens, int64_t K, double* work, float* x_mean, float* x_sq,
                  void* stream);
int awq_weight_colsum(const void* w, int dtype, int64_t rows, int64_t K, int64_t group_size, float* gmax_work,
                      double* partial, void* stream);
/* out[k] = fp32(sum_{b < nblk, ascending} partial[b * K + k] / divisor) (fp64 sum) */
int awq_column_mean(const double* partial, int64_t nblk, int64_t K, double divisor, float* out, void* stream);
/* RTN of W * diag(col_scale) in one pass — the packed outputs of awq_apply_input_scale into a
 * copy followed by awq_quantize_groups on the copy, bit for bit, without the copy (the
 * activation-aware search's last step, round 5).  bf16 / fp16 / fp32 2-D w [rows, K],
 * group_size 32 / 64 / 128 / 256 with K % group_size == 0 and K % 8 == 0, w and col_scale
 * 16-B aligned, packed outputs only (NULL = not wanted); otherwise AWQ_EINVAL (make the two
 * calls).  (ABI 16) */
int awq_quantize_groups_scaled(const void* w, int dtype, int64_t rows, int64_t K, int32_t group_size, int bits,
                               int symmetric, const float* col_scale, int32_t* qweight, int32_t* qzeros,
                               uint16_t* scales, void* stream);
/* table fp32 [n_grid, K]; w_mean NULL = no duo scaling */
int awq_act_scale_table(const float* x_mean, const float* w_mean, int64_t K, int n_grid, float* table,
                        void* stream);
/* The same table (bit for bit) with a caller workspace: every (candidate, channel) power is
 * evaluated once, by one thread, the raw values kept in work between a pass that forms each
 * 256-channel slice's max / min and one that normalises (awq_act_scale_table recomputes the
 * normaliser's pass in each of its workgroups: ~10x the fp64 work, on n_grid x 8 CUs).
 * work fp64 [n_grid * (K + 3 * ceil(K / 256))].  (ABI 16) */
int awq_act_scale_table_ws(const float* x_mean, const float* w_mean, int64_t K, int n_grid, double* work,
                           float* table, void* stream);
/* rtable [n_grid, K] = RN_f32(1 / table) where table is in [2^-60, 2^60], else a NaN (ABI 17;
 * was 0): lets the loss kernel form fp32(dq / s) as one Markstein-corrected product (exact there:
 * awq_selftest 1); a quotient through an out-of-range entry is NaN, and a wave whose candidate
 * loss comes out NaN redoes that candidate with IEEE divisions (the same bits in range). */
int awq_act_recip_table(const float* table, int n_grid, int64_t K, float* rtable, void* stream);
/* rtable: awq_act_recip_table's output for the same table, or NULL (IEEE divisions).
 * Precondition: every table entry is positive and finite, as awq_act_scale_table produces
 * (it maps inf / NaN to 1).  The kernel relies on it — RN(w * s) is NaN exactly when w is, so
 * the weights' NaN flag is taken once per group — and does not check a caller's own table. */
int awq_act_search_losses(const void* w, int dtype, int64_t rows, int64_t K, int64_t group_size, int bits,
                          int symmetric, const float* table, const float* rtable, int n_grid, const float* x_sq,
                          float* part, int64_t part_stride, void* stream);
/* losses fp64 [n_grid], best int32 [1], s_best fp32 [K] (any may be NULL) */
int awq_act_search_select(const float* part, int n_grid, int64_t part_stride, const float* table, int64_t K,
                          double* work, double* losses, int32_t* best, float* s_best, void* stream);
/* out [rows, K] (dtype D) = RN_D(w * s[k]) */
int awq_apply_input_scale(const void* w, int dtype, int64_t rows, int64_t K, const float* s, void* out,
                          void* stream);

/* ---- Activation-aware clip search (additive to ABI 17): the second step of AutoAWQ's published
 * method, with the scale search's diagonal loss.  Not in the reference (see above).  For one
 * weight W [rows, K] of dtype D (bf16 / fp16 / fp32), a column scale s = col_scale fp32 [K]
 * (positive and finite, as awq_act_scale_table produces; not checked), the statistics x_sq fp32
 * [K], and 1 <= n_candidates <= n_grid; every step reuses arithmetic pinned above:
 *   w' = RN_D(w * s[k])                                   (awq_apply_input_scale)
 *   [mn, mx] of each group of w' as RTN takes it (awq.py:192-199: after the symmetric
 *       abs-max; a NaN in the group makes both NaN)
 *   candidate i = 0 .. n_candidates-1: alpha_i = RN_f32((n_grid - i) / n_grid), the range
 *       RN_D(RN_f32(mn * alpha_i)), RN_D(RN_f32(mx * alpha_i))      (awq_quantize_search)
 *   scale / zero point of the shrunk range exactly as RTN      (awq.py:202-211)
 *   per element: q (awq.py:245-248) of w'; dq = fp16(fp16(q - z) * fp16(scale));
 *       d = RN_f32(dq / s[k]) - w (against the ORIGINAL w); c = x_sq[k] * (d * d), every op
 *       rounded to fp32, no contraction                      (awq_act_search_losses)
 *   group loss: each 8-element chunk summed in order from +0, then the pairwise tree over the
 *       chunks, adjacent pairs first                         (awq_quantize_search's order)
 *   winner: the first strict minimum; a NaN loss never wins; NaN / inf groups and ties keep
 *       i = 0.  qweight / qzeros / scales = RTN of w' with the winner's range.
 * Hence: n_candidates = 1 gives awq_quantize_groups_scaled's bits; s = 1 and x_sq = 1 give
 * awq_quantize_search's; every group's candidate-0 loss is awq_act_search_losses' partial for
 * the one-row table [1, K] = s.
 * col_rscale: awq_act_recip_table(col_scale, 1, K) (entries NaN outside [2^-60, 2^60]), or NULL;
 *   NULL, or a loss that comes out NaN, means the IEEE division — the same bits either way.
 * best_idx int32 [rows * G] (the winners) and group_loss fp32 [2, loss_stride] (row 0: candidate
 *   0's loss of every group, row 1: the winner's; this weight's groups at [0, rows * G), so the
 *   linears of a layer group write one buffer at their own offsets, and
 *   awq_act_search_select(group_loss, 2, loss_stride, ...) returns the layer group's fp64 loss
 *   before and after clipping) may be NULL; at least one output must be given.
 * Kernels, the same bits: group_size 32 / 64 / 128 / 256 with 16-B aligned w, col_scale,
 * col_rscale and x_sq: the streaming kernel (one wave per 2048 elements; when G % (32 / bits)
 * != 0 it first zeroes qzeros on the stream); any other power-of-two group_size in [8, 512]
 * dividing K, or element-aligned pointers: one wave per group.  Anything else (fp64, larger or
 * other group sizes, K % group_size != 0): AWQ_EUNSUPPORTED.  Packed outputs only. */
int awq_quantize_clip_scaled(const void* w, int dtype, int64_t rows, int64_t K, int32_t group_size, int bits,
                             int symmetric, const float* col_scale, const float* col_rscale, const float* x_sq,
                             int n_grid, int n_candidates, int32_t* qweight, int32_t* qzeros, uint16_t* scales,
                             int32_t* best_idx, float* group_loss, int64_t loss_stride, void* stream);

/* ---- Clip search with the token-sample loss (additive to ABI 17): awq_quantize_clip_scaled's
 * candidates scored by the published objective (AutoAWQ _compute_best_clip), the error at the
 * linear's output on calibration samples x [T, K] (dtype D of w, row stride x_row_stride >= K
 * elements: the unscaled samples, as awq_output_error takes them).  Every step reuses arithmetic
 * pinned above:
 *   w', each group's [mn, mx], alpha_i, the shrunk range, its scale and zero point, q and dq:
 *       awq_quantize_clip_scaled's, for the candidates cand_begin <= i < cand_begin + n_candidates
 *       <= n_grid.  Hence, for the same i, a group's packed bits are those
 *       awq_quantize_clip_scaled writes.
 *   d = RN_f32(RN_f32(dq / s[k]) - fp32(w)), against the ORIGINAL w, no contraction
 *       (awq_output_error's d with col_scale = s); col_rscale as in awq_quantize_clip_scaled: the
 *       same bits as the IEEE division.
 *   loss of (row n, group g, candidate i): E[t] = sum_{k in g} d[n, k] x[t, k], loss = sum_t E[t]^2.
 * Accuracy: the order of the sum over k is the implementation's, so the contract is awq_output_error's
 * bound with the group size L for K: |E - E_exact| <= eps_L * sum_{k in g} |d| |x|, eps_L = 2^-17 +
 * L 2^-22 (L 2^-22 alone where the operands are f32: the generic kernel); the sum over t adds at most
 * (T + 1) 2^-24 relative.  No floating-point atomics: a (row, group, candidate) loss is formed in one
 * place, the tokens in a fixed order — the same bits from run to run.
 * Winner: the first strict minimum OF THE fp32 LOSSES AS RETURNED; a NaN loss never wins; NaN / inf
 * groups and ties keep the first candidate (cand_begin).
 * Outputs (each may be NULL, at least one must be given):
 *   qweight / qzeros / scales: RTN of w' with the winner's range (qzeros is zeroed on the stream
 *       first, then every group ORs its field in);
 *   best_idx int32 [rows * G]: the winners' absolute candidate indices;
 *   group_loss fp32 [2, loss_stride]: row 0 the loss of candidate cand_begin, row 1 the winner's —
 *       the layout awq_act_search_select(group_loss, 2, loss_stride, ...) reads;
 *   cand_loss fp32 [n_candidates, loss_stride]: every candidate's loss, row i - cand_begin.
 *   This weight's groups sit at [0, rows * G) of every row; loss_stride >= rows * G.
 * n_candidates = 1 forces candidate cand_begin for every group (cand_begin = 0:
 * awq_quantize_groups_scaled's bits).
 * Checked in this order, before any launch (the pointers are not looked at until the last two):
 * bits other than 4 / 8, group_size <= 0, a negative rows / K / T: AWQ_EINVAL; a group_size that is
 * not a power of two in [8, 512], K % group_size != 0, fp64: AWQ_EUNSUPPORTED; another dtype code,
 * x_row_stride < K, n_grid < 1, n_candidates < 1, cand_begin < 0 or cand_begin + n_candidates >
 * n_grid: AWQ_EINVAL; rows K, rows T or T x_row_stride above 2^60, rows G >= 2^31: AWQ_EUNSUPPORTED;
 * no output: AWQ_EINVAL; rows == 0 or K == 0: AWQ_OK, nothing is read or written; a NULL w /
 * col_scale (x when T > 0), a short loss_stride, a misaligned pointer: AWQ_EINVAL.
 * T == 0: every loss is +0, every winner cand_begin.
 * Kernels: bf16 with group_size 32 / 64 / 128 / 256, 16-B aligned w / x / col_scale / col_rscale,
 * x_row_stride % 8 == 0 (and K, x_row_stride < 2^22): v_mfma_f32_32x32x16_bf16 on the hi / lo split
 * of d, 128 rows of one group per workgroup; everything else: one wave per group on f32 operands.
 * `work` is not used (awq_quantize_clip_output_work_bytes returns 0): it may be NULL. */
int64_t awq_quantize_clip_output_work_bytes(int64_t rows, int64_t K, int64_t group_size, int64_t T, int n_candidates);
/* 1 if a call with these arguments (already accepted by the checks above) takes the MFMA kernel, else
 * 0: the predicate the entry itself routes by.  Host only, nothing is dereferenced. */
int awq_quantize_clip_output_fast(const void* w, int dtype, int64_t K, int64_t group_size, const float* col_scale,
                                  const float* col_rscale, const void* x, int64_t x_row_stride);
int awq_quantize_clip_output(const void* w, int dtype, int64_t rows, int64_t K, int64_t group_size, int bits,
                             int symmetric, const float* col_scale, const float* col_rscale,
                             const void* x, int64_t T, int64_t x_row_stride,   /* samples [T, K] of `dtype` */
                             int n_grid, int cand_begin, int n_candidates,
                             int32_t* qweight, int32_t* qzeros, uint16_t* scales, int32_t* best_idx,
                             float* group_loss, float* cand_loss, int64_t loss_stride, void* work, void* stream);

/* ---- Scale folding (additive to ABI 17).  A searched weight is W * diag(s): it is usable only
 * once 1 / s is folded into whatever produces its input — the preceding norm's weight, or the
 * rows (and bias) of the preceding linear.  This is that fold, for rows:
 *   out[r, k] = RN_D( RN_f32( fp32(w[r, k]) / row_scale[r] ) )
 * w, out [rows, K] of dtype D (bf16 / fp16 / fp32; anything else: AWQ_EUNSUPPORTED); row_scale
 * fp32 [rows].  The division is the IEEE fp32 division (correctly rounded), its quotient rounded
 * once, to nearest-even, into D — torch's CPU result of (w.float() / s[:, None]).to(D).
 * row_scale is not checked (positive and finite when it comes from awq_act_scale_table);
 * non-finite values propagate as IEEE defines, NaN payloads are unspecified.
 * out == w is allowed (in place); any other overlap is the caller's error.  Checked in this
 * order, nothing launched on a failure: negative rows or K: AWQ_EINVAL; the dtype; rows == 0 or
 * K == 0: AWQ_OK without a launch (the pointers are not looked at: an empty tensor's may be
 * null); rows * K > 2^60: AWQ_EINVAL; a null pointer: AWQ_EINVAL.
 * A 1-D vector (a norm weight, a bias) is rows = n, K = 1.
 * Kernels, the same bits: w and out 16-B aligned and K % 8 == 0: the streaming structure (one
 * wave per 2048 consecutive elements, 16-B loads and stores, every 8-element chunk inside one
 * row, the row taken from the element offset); anything else (any K, K = 1, element-aligned
 * pointers): one element per lane.  Offsets are 64-bit throughout. */
int awq_fold_rows(const void* w, int dtype, int64_t rows, int64_t K, const float* row_scale, void* out,
                  void* stream);

/* ---- Calibration pass (additive to ABI 17): the statistics awq_act_stats defines, taken while a
 * model runs.  Every linear of a decoder block reads the output of a memory-bound op; these three
 * entries produce that output where it is ours to produce (RMSNorm, the SwiGLU product) and add its
 * column sums to fp64 running sums, micro-batch after micro-batch:
 *   acc_abs[k] += sum_t |v[t,k]|,  acc_sq[k] += sum_t v[t,k]^2        (fp64 [K], caller-zeroed)
 * in awq_act_stats' order continued across calls: t ascending inside 32-token sub-blocks, the
 * sub-blocks ascending inside 256-token blocks, the blocks' sums added ascending onto the running
 * value.  The caller guarantees that every call on an accumulator but the last has
 * tokens % 256 == 0 and passes the number of tokens already added as tokens_before; a call with
 * tokens_before % 256 != 0 is refused (AWQ_EINVAL, nothing launched).  After the last call
 *   awq_column_mean(acc_abs, 1, K, T, x_mean),  awq_column_mean(acc_sq, 1, K, T, x_sq)
 * (T = all tokens) give the bits of awq_act_stats on the concatenated rows.
 * dtype D: bf16 / fp16 / fp32 (else AWQ_EUNSUPPORTED).  Checked in this order, nothing launched on
 * a failure: the dtype; a negative tokens, K or tokens_before: AWQ_EINVAL; tokens == 0 or K == 0:
 * AWQ_OK without a launch (the pointers are not looked at); tokens_before % 256; tokens > 65535 *
 * 256 or K > 2^31: AWQ_EINVAL; row_stride < K; null pointers.  Caller-owned device memory, the
 * caller's stream, no allocation, no synchronisation.
 *
 * awq_act_stats_accum: v = x [tokens, K] with a row stride in elements >= K (a column slice or
 *   any other row-strided view).  work fp64 [2 * ceil(tokens / 256) * K].
 * awq_rmsnorm_stats: transformers' LlamaRMSNorm with its roundings; x, out [tokens, H]
 *   contiguous, weight [H] of dtype D, eps fp32:
 *     v_t = sum_k RN_f32(x[t,k]^2) in fp32, in this order: the row is cut into 8-element chunks
 *           c = 0 .. ceil(H/8)-1, each summed in order from +0; slot l (0..63) adds the sums of
 *           chunks l, l + 64, l + 128, ... ascending from +0; v_t is the pairwise tree over the
 *           64 slots, adjacent pairs first (awq_quantize_search's tree)
 *     r_t = RN_f32(1 / RN_f32(sqrt(RN_f32(RN_f32(v_t / H) + eps))))   (IEEE / and sqrt)
 *     out[t,k] = RN_D(weight[k] * RN_D(RN_f32(x[t,k] * r_t)))
 *   and v = out.  acc_abs = acc_sq = NULL: the norm alone.  out may not alias x (x is read twice);
 *   H <= 2^24.  work fp64 [ceil(tokens / 2) + 2 * ceil(tokens / 256) * H] (the first ceil(tokens/2)
 *   hold r_t as fp32 and are all that the norm alone needs).
 * awq_swiglu_stats: gate, up [tokens, K] with one row stride >= K (two column halves of a fused
 *   [tokens, 2K] buffer), out [tokens, K] contiguous, overlapping neither input:
 *     out = RN_D(RN_D(silu(g)) * u),  silu(g) = RN_f32(g / RN_f32(1 + expf(-g))) in fp32
 *   and v = out.  expf is the device math library's (<= 1 ulp), not bit-reproducible elsewhere: out
 *   is specified to 1 ulp of D (bf16 / fp16) of the fp64 expression, the sums exactly on the out
 *   that was written.  g below -88.7 (expf overflows) gives -0 where the exact value is within
 *   1e-36 of it.  acc_abs = acc_sq = NULL: the product alone (work is not looked at).
 *   work fp64 [2 * ceil(tokens / 256) * K].
 * Kernels, the same bits: K % 8 == 0, row strides % 8 == 0 and 16-B aligned pointers: 256-token x
 * 32-column tiles with 16-B accesses; anything else: one lane per column and block. */
int awq_act_stats_accum(const void* x, int dtype, int64_t tokens, int64_t K, int64_t row_stride,
                        int64_t tokens_before, double* work, double* acc_abs, double* acc_sq, void* stream);
int awq_rmsnorm_stats(const void* x, int dtype, int64_t tokens, int64_t H, const void* weight, float eps, void* out,
                      int64_t tokens_before, double* work, double* acc_abs, double* acc_sq, void* stream);
int awq_swiglu_stats(const void* gate, const void* up, int dtype, int64_t tokens, int64_t K, int64_t row_stride,
                     void* out, int64_t tokens_before, double* work, double* acc_abs, double* acc_sq, void* stream);

/* ---- Logit comparison (additive to ABI 17; beyond the reference): the tail of a model-level
 * evaluation.  ref and q are logits [T, V] of dtype D = bf16 / fp16 / fp32, each with its own row
 * stride in elements (>= V).  Per row t, a = fp32(ref[t, .]), b = fp32(q[t, .]), m_r = max_v a_v:
 *   S_r = sum_v exp(a_v - m_r),  lse_r = m_r + log S_r           (S_q, lse_q likewise from b)
 *   nll_ref[t] = lse_r - a[targets[t]],  nll_q[t] = lse_q - b[targets[t]]
 *       targets[t] < 0: not scored, both +0;  targets[t] >= V: both NaN
 *   kl[t] = (A / S_r - lse_r) + lse_q,  A = sum_v exp(a_v - m_r) (a_v - b_v)
 *       = KL(softmax a || softmax b), as computed: no clamp, it may be negative within the bound below
 *   argmax_ref[t], argmax_q[t] = the LOWEST index attaining the row's maximum
 * A row of ref that holds a NaN or +-inf: nll_ref[t] = kl[t] = NaN, argmax_ref[t] = -1; a row of q
 * likewise for nll_q, kl, argmax_q.  Nothing else is masked and no row affects another.
 * q = NULL: the single-model form (nll_ref and argmax_ref only; q_row_stride, nll_q, kl and argmax_q
 * are not looked at).  targets = NULL: no nll output.  Any output pointer may be NULL.
 * lse_r and lse_q come from one instruction sequence: bit-identical rows of ref and q give
 * nll_q == nll_ref bit for bit and kl[t] == +0.
 *
 * Order (fixed; the same bits from run to run, for any T, on either path; no atomics).  One
 * 256-thread workgroup per row.  The row is cut into 8-element chunks c = 0 .. ceil(V/8)-1; thread
 * i takes chunks i, i + 256, ... ascending and keeps (m, S, A), starting from (-inf, +0, +0).  Per
 * chunk: cm = the chunk's maximum; if cm > m: e = expf(m - cm), m = cm, else e = 1;
 * w_j = expf(x_j - m); S = S e + (((0 + w_0) + w_1) + ... + w_7); A = A e + (((0 + w_0 d_0) + ...) +
 * w_7 d_7), d_j = a_j - b_j (elements past V add +0).  Then M = the maximum of the threads' m;
 * thread i contributes S f, A f with f = 1 if its m == M, else expf(m - M); the 256 contributions
 * are added as the pairwise tree over the 64 threads of each wave, adjacent pairs first
 * (awq_quantize_search's tree), then (w0 + w1) + (w2 + w3) over the four waves.  lse = M + logf(S).
 * One online pass: each matrix is read once.
 *
 * Error contract (fp64 evaluation of the definitions on the same inputs), per scored finite row:
 *   |nll - nll64| <= (D + C + c0) 2^-24 + 2^-23 |lse| + 2^-24 |nll|
 *   |kl - kl64|   <= (D + C + c0) 2^-23 (1 + M1) + 3 2^-24 (M1 + |lse_r| + |lse_q|),
 *                    M1 = sum_v p_v |a_v - b_v|, p = softmax a
 * with
 *   D  = 104: a term with x_v - M < -104 is flushed (e^-104 < 2^-149), one above it carries the
 *        rounding of its exponent: the exponents x - m, m - m', ..., m'' - M of the factors a term
 *        passes through all have one sign and add up to x_v - M, so together they are wrong by at
 *        most 2^-24 |x_v - M| <= D 2^-24, which is the term's relative error;
 *   C  = 4 n + 20, n = ceil(ceil(V / 8) / 256) chunks per thread: the roundings a term passes after
 *        its own expf, in units of 2^-24 relative: <= 8 additions of the chunk sum, per later chunk
 *        of the thread one rescale (expf <= 1 ulp = 2, the product 1) and one addition, the rescale
 *        to M (3), 8 additions of the tree, one spare;
 *   c0 = 48: the term's own expf (2), logf <= 1 ulp of |log S| <= 2^-23 ln 2^31 (44), and 2 for what
 *        the flushed terms (< 2^31 2^-149 of S >= 1) and second-order products add.
 *   The three further terms: the addition M + log S (2^-24 |lse|), its fp64 counterpart's inputs
 *   (none) and the final subtraction, whose result is rounded to fp32: 2^-24 |nll|, |nll| <= |lse| +
 *   |a_target| (without it no fp32 output could meet the bound when |a_target| >> |lse|).
 *   kl: A / S_r is a p-weighted mean of d_v whose weights carry (D + C + c0) 2^-24 twice (numerator
 *   and S_r), the two lse their bound above, the two final additions <= 2^-24 (2 M1 + 3 |lse_r| +
 *   2 |lse_q|).  expf / logf are the device math library's (<= 1 ulp).
 *
 * Kernels, the same bits: 16-B aligned bases and row strides % 8 == 0 (fp32: % 4): 16-B loads, the
 * ragged last chunk element by element; anything else: every chunk element by element.
 * Checked in this order, nothing launched on a failure: the dtype (AWQ_EUNSUPPORTED); T < 0 or V < 1
 * (AWQ_EINVAL); T == 0: AWQ_OK, no pointer is looked at; V >= 2^31; ref == NULL; a row stride < V;
 * T x row stride > 2^60 (all AWQ_EINVAL).  More than 65536 rows: the grid is capped and a workgroup
 * takes rows blockIdx, blockIdx + grid, ...  Caller-owned device memory, the caller's stream, no
 * workspace, no allocation, no synchronisation. */
int awq_logit_compare(const void* ref, const void* q, int dtype, int64_t T, int64_t V,
                      int64_t ref_row_stride, int64_t q_row_stride, const int64_t* targets,
                      float* nll_ref, float* nll_q, float* kl,
                      int32_t* argmax_ref, int32_t* argmax_q, void* stream);

/* Device self-test (diagnostics).  which = 0: the fast reciprocal used by the streaming
 * kernel against IEEE 1/s over every bf16 s >= RN_bf16(1e-10); which = 1: the loss kernel's
 * Markstein quotient against the IEEE division for every s in [1, 2) and every positive
 * finite fp16 dividend; which = 2: the fp16 reciprocal (rcp + one Newton step) against IEEE
 * 1/s over every positive finite fp16 s; adds the number of mismatches to *result (device
 * unsigned long long, caller-zeroed). */
int awq_selftest(int which, unsigned long long* result, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AWQ_HIP_H */
