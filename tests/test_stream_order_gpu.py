"""Every kernel entry point off the default stream (include/awq_hip.h: "launches are asynchronous on
that stream, nothing synchronises", "one stream per call"; tests/stream_gate.py).

The legacy default stream serialises with everything, so the rest of the suite cannot see a launch,
a memset or a later stage of a multi-launch entry that goes to the wrong stream.  Here
  1. the arena cases of the other files run again under stream_gate.ordered(): one case per kernel
     path and per internal launch sequence, at the smallest shape their files use, each asserting
     everything it asserts there (guards, every output byte against the CPU expectation, both fill
     polarities) on a stream whose memory only becomes right behind a device-side gate;
  2. every launching wrapper of awq_quantizer/_hip.py returns, under the same protocol, the bits
     it returns on the default stream ("the same on any stream"; that result is pinned elsewhere);
  3. the class API does, and a PackedBatch built on one stream runs on another;
  4. two host threads on two streams make 200 calls each into the multi-launch entries.
A case whose gate had ended before stream 0 was synchronised raises stream_gate.GateUnproven: an
error naming the case, never a pass.

The file's name sorts it after every other file with GPU tests: it re-runs their case functions and
starts threads and a dozen streams, so it goes last and no earlier test's place in a run moves.

Left out: awq_selftest as an arena case (it adds zero mismatches to a caller-zeroed counter: a
misplaced run is invisible), the awq_stream_* pipeline and awq_runtime_warmup (they own their
streams; test_cli.py covers them)."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import stream_gate
import test_gpu_autoawq_import as imp
import test_gpu_bounds as tb
import test_gpu_calib_kernels as ck
import test_gpu_clip_output as co
import test_gpu_output_error as oe
from test_gpu_bounds import BF16, F16, F32, F64, I32, Call

pytestmark = pytest.mark.gpu


def _dev():
    return tb._dev()


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def walk(cases):
    """Every (label, fn, args) under one ordered() context.  A failed assertion does not stop the
    walk and the failure names every failing case; any other error (an unproven gate, a HIP error)
    ends it at once: nothing more is launched after it."""
    dev = _dev()
    failed = []
    with stream_gate.ordered(dev) as st:
        for label, fn, args in cases:
            st.case = label
            before = st.gates
            try:
                fn(*args)
            except AssertionError as e:
                failed.append(f"{label}: {e}")
            else:
                assert st.gates > before, f"{label}: ran no gated call"
        ms, where = st.longest_span_ms()
        print(f"{st.gates} gates of {st.gate_ms} ms ({st.streams_skipped} stream(s) skipped); the longest span to the "
              f"stream-0 synchronise: {ms:.3f} ms ({where})")
    assert not failed, "\n\n".join(failed)


# ---------------------------------------------------------------- 0. the precondition
def test_default_stream_does_not_wait_for_the_gate():
    """The gate on S, a torch op on the default stream, synchronised: the gate must still be
    running.  If not, the default stream waits for S on this runtime and no case below can prove
    anything — a failure, not a skip.  The calibration is checked with it: the gate, timed, lasts
    about GATE_MS."""
    dev = _dev()
    with torch.cuda.stream(torch.cuda.default_stream(dev)):
        torch.ones(64, device=dev) * 2                  # (the op's code loads at its first launch, not behind the gate)
    with stream_gate.ordered(dev) as st:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st.stream)
        done = st.gate()
        b.record(st.stream)
        with torch.cuda.stream(torch.cuda.default_stream(dev)):
            x = torch.ones(64, device=dev) * 2
        torch.cuda.default_stream(dev).synchronize()
        assert not done.query(), "the default stream waited for the gate's stream: no case can prove anything"
        st.stream.synchronize()
        assert done.query() and float(x.sum()) == 128.0
        ms = a.elapsed_time(b)
        print(f"gate of {st.gate_ms} ms ({st.cycles} cycles) lasted {ms:.2f} ms; {st.streams_skipped} fresh stream(s) "
              f"skipped for sharing stream 0's queue")
        assert 0.5 * st.gate_ms <= ms <= 3 * st.gate_ms


# ---------------------------------------------------------------- 1. the arena cases
def test_order_quantize():
    walk([("groups_ex streaming byte tiles", tb.test_quantize_streaming, ("byte", (3, 1024), 128, BF16, 4, False)),
          ("groups_ex streaming padded rows", tb.test_quantize_streaming, ("pad", (5, 200), 128, F16, 8, True)),
          ("groups_ex row segment", tb.test_quantize_row_segment, ((4, 250), 100, BF16, 4, False)),
          ("groups_ex generic fp64", tb.test_quantize_generic, (F64, (3, 200), 64, 0, 4, False)),
          ("groups_ex generic gs 1024", tb.test_quantize_generic, (BF16, (2, 2088), 1024, 0, 4, True)),
          ("groups_ex small tensor", tb.test_quantize_small_tensor, (BF16, 4, False, False)),
          ("search_ex", tb.test_quantize_search, (BF16, (3, 1024), 128, 4, False))])


def test_order_ragged():
    """The descriptors and the block table are pointer-bearing: never stale."""
    walk([(f"ragged search={s} table={t}", tb.test_quantize_ragged, (BF16, 4, False, s, t))
          for s in (None, (4, 3)) for t in (True, False)])


def test_order_params_dequant_pack():
    walk([("group_params_ex", tb.test_group_params, (BF16, 4, False, 0, "both")),
          ("apply_params mode 0", tb.test_apply_params, (BF16, 4, False, 0, 64)),
          ("apply_params mode 1", tb.test_apply_params, (BF16, 4, False, 1, 64)),
          ("apply_params_ex int32 fp16 ops", tb.test_apply_params_ex_int32_with_fp16_ops, (64,)),
          ("dequantize", tb.test_dequantize, ((3, 1024), 128, 4, False, BF16, False, 0)),
          ("dequantize_packed", tb.test_dequantize, ((3, 1024), 128, 4, False, BF16, True, 0)),
          ("pack_rows", tb.test_pack_rows, (9, 4, 0))])


def test_order_export_import():
    walk([("export_autoawq_gemm both kernels", tb.test_export_autoawq_gemm, (72, 512, 64, 0, True)),
          ("import_autoawq_gemm all outputs", imp.test_guard_bands, (72, 384, 128, 0, "all"))])


def test_order_error_reports():
    """quant_error with totals: memset, kernel, block, final; output_error: MFMA or generic, then
    the sum kernel."""
    dev = _dev()
    walk([("quant_error streaming totals", tb.test_quant_error, ((3, 1024), 128, BF16, 4, False, True)),
          ("quant_error streaming no totals", tb.test_quant_error, ((3, 1024), 128, BF16, 4, False, False)),
          ("quant_error group totals", tb.test_quant_error, ((4, 250), 100, BF16, 4, False, True)),
          ("quant_error group no totals", tb.test_quant_error, ((4, 250), 100, BF16, 4, False, False)),
          ("output_error bf16 aligned (MFMA)", oe._guard_bands, (dev, BF16, 0, True, True)),
          ("output_error fp16 skewed (generic)", oe._guard_bands, (dev, F16, 2, True, True))])


def test_order_act_search():
    walk([("act_stats two blocks", tb.test_act_stats, (257, 264, BF16)),
          ("weight_colsum one pass + column_mean", tb.test_weight_colsum_and_column_mean, (128, BF16)),
          ("weight_colsum two pass + column_mean", tb.test_weight_colsum_and_column_mean, (16, BF16)),
          ("act_scale_table, _ws, recip_table", tb.test_act_scale_and_recip_tables, (264, 5, True)),
          ("act_search_losses ring gs 128", tb.test_act_search_losses, (F16, 128, 8, True, True)),
          ("act_search_losses ringless gs 512", tb.test_act_search_losses, (F32, 512, 4, True, True)),
          ("act_search_select", tb.test_act_search_select, (1025, 5, None)),
          ("apply_input_scale", tb.test_apply_input_scale, (BF16, 0)),
          ("quantize_groups_scaled", tb.test_quantize_groups_scaled, ((23, 384), BF16, 4, False))])


def test_order_clip():
    """Both clip searches; the streaming cases have G % (32 / bits) != 0, so the qzeros memset runs."""
    dev = _dev()
    walk([("clip_scaled streaming, zeroed qzeros", tb.test_quantize_clip_scaled,
           ("zeroed_qzeros", (23, 384), 128, 0, 0, "all", BF16, 4, False)),
          ("clip_scaled group kernel", tb.test_quantize_clip_scaled, ("per_group", (4, 256), 16, 0, 0, "all", BF16, 4, False)),
          ("clip_output bf16 gs 128 (MFMA)", co._guard_bands, (dev, BF16, 128, 4, False, co.OUTS[0], 0)),
          ("clip_output fp16 gs 16 (generic)", co._guard_bands, (dev, F16, 16, 4, False, co.OUTS[0], 0))])


def test_order_fold():
    walk([("fold_rows streaming", tb.test_fold_rows, ((3, 1024), 0, False, BF16)),
          ("fold_rows any K", tb.test_fold_rows, ((3, 13), 0, False, BF16)),
          ("fold_rows in place", tb.test_fold_rows, ((5, 264), 0, True, BF16))])


def test_order_helpers():
    walk([("stream_copy", tb.test_stream_copy, (16,)),
          ("stream_ceiling", tb.test_stream_ceiling, (4096,)),
          ("dequant_ceiling", tb.test_dequant_ceiling, (16,))])


# ---- the calibration entries as Call cases (their guard tests use Arena directly)
CALIB_T = ck.GUARD_T        # 270: two blocks, the second partial


def seeded_sums(v, seed_abs, seed_sq):
    """The running sums after one call on accumulators that held the seeds: each 256-token block's
    sums (ck.expected_sums of the block: 0 + the block) added ascending onto the running value."""
    a, q = seed_abs.clone(), seed_sq.clone()
    for b0 in range(0, v.shape[0], 256):
        ba, bq = ck.expected_sums(v[b0:b0 + 256])
        a, q = a + ba, q + bq
    return a, q


def _seeds(K):
    k = torch.arange(K, dtype=F64)
    return 3.0 + 0.125 * k, 1.0e3 + k * k


def calib_accum(K):
    dev, hip = _dev(), ck._hipmod()
    x = ck.rows(CALIB_T, K, BF16, 3)
    sa, sq = _seeds(K)
    ea, es = seeded_sums(x, sa, sq)
    c = Call(dev, seed=K)
    xb = c.inp("x", x)
    wk = c.work("work", 8 * hip.calib_work_size(CALIB_T, K))
    ab = c.inp("acc_abs", sa, untouched=False, expect=ea, nan_dtype=F64)
    qb = c.inp("acc_sq", sq, untouched=False, expect=es, nan_dtype=F64)
    c.build()
    c.run(lambda: hip.load_library().awq_act_stats_accum(xb.ptr, hip.AWQ_DTYPE[BF16], CALIB_T, K, K, 0, wk.ptr, ab.ptr,
                                                         qb.ptr, _stream(dev)))


def calib_rmsnorm(K):
    """rms_rows_kernel, the norm kernel, acc_add_kernel."""
    dev, hip = _dev(), ck._hipmod()
    x, w = ck.norm_case(CALIB_T, K, BF16, 4)
    ref = ck.rmsnorm_ref(x, w, 1e-5)
    sa, sq = _seeds(K)
    ea, es = seeded_sums(ref, sa, sq)
    c = Call(dev, seed=K + 1)
    xb, wb = c.inp("x", x), c.inp("weight", w)
    ob = c.out("out", ref, nan_dtype=BF16)
    wk = c.work("work", 8 * hip.calib_work_size(CALIB_T, K, norm=True))
    ab = c.inp("acc_abs", sa, untouched=False, expect=ea, nan_dtype=F64)
    qb = c.inp("acc_sq", sq, untouched=False, expect=es, nan_dtype=F64)
    c.build()
    c.run(lambda: hip.load_library().awq_rmsnorm_stats(xb.ptr, hip.AWQ_DTYPE[BF16], CALIB_T, K, wb.ptr, 1e-5, ob.ptr, 0,
                                                       wk.ptr, ab.ptr, qb.ptr, _stream(dev)))


def calib_swiglu(K):
    """out is specified to 1 ulp of the float64 expression (expf is the device library's): the
    expectation is the kernel's own product, asserted to be within that ulp first; the sums are
    exact on the out that was written."""
    dev, hip = _dev(), ck._hipmod()
    gate, up = ck.swiglu_case(CALIB_T, K, BF16, 6)
    out, _ = ck.run_swiglu(hip, gate, up, dev, strided=False)
    s64, u64 = ck.silu64_product(gate, up)
    with np.errstate(all="ignore"):
        ref = ck.round64(ck.round64(s64, BF16) * u64, BF16)
    assert int(ck.ulp_distance(out, ref).max()) <= 1
    sa, sq = _seeds(K)
    ea, es = seeded_sums(out, sa, sq)
    c = Call(dev, seed=K + 2)
    gb, ub = c.inp("gate", gate), c.inp("up", up)
    ob = c.out("out", out, nan_dtype=BF16)
    wk = c.work("work", 8 * hip.calib_work_size(CALIB_T, K))
    ab = c.inp("acc_abs", sa, untouched=False, expect=ea, nan_dtype=F64)
    qb = c.inp("acc_sq", sq, untouched=False, expect=es, nan_dtype=F64)
    c.build()
    c.run(lambda: hip.load_library().awq_swiglu_stats(gb.ptr, ub.ptr, hip.AWQ_DTYPE[BF16], CALIB_T, K, K, ob.ptr, 0,
                                                      wk.ptr, ab.ptr, qb.ptr, _stream(dev)))


def test_order_calibration():
    """K 8: the 16-B tiles; K 12: one lane per column.  Statistics on, the accumulators seeded
    non-zero (inputs that are also outputs)."""
    walk([(f"{fn.__name__} K={K}", fn, (K,)) for fn in (calib_accum, calib_rmsnorm, calib_swiglu) for K in (8, 12)])


# ---------------------------------------------------------------- 2. the _hip.py wrappers
def _randn(shape, dtype, seed, scale=0.03):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _pos(n, seed):
    return torch.exp2(torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 4 - 2).float()


def _packed_of(dev, w, gs, bits, sym):
    """(qweight, qzeros, scales) of w on the device, from the CPU oracle."""
    rows, K = w.shape
    e = tb.quant_expect(w, rows, K, gs, bits, sym)
    return e["qweight"].to(dev), e["qzeros"].to(dev), e["scales"].to(dev)


def wrapper_cases(hip, dev):
    """name -> make(seed) -> (tensors the call reads, pointer-bearing tensors, call).  Every call
    fills the outputs it hands in with junk bytes first (on its stream), so none starts from an
    earlier run's bytes and a memset that the entry owes is seen when it goes elsewhere."""
    R, K, gs, bits = 3, 1024, 128, 4
    G, per = K // gs, 32 // bits
    cases = {}

    def junk(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=dev)
        t.view(-1).view(torch.uint8).fill_(co.JUNK)
        return t

    def case(fn):
        cases[fn.__name__] = fn
        return fn

    def packed_outs(rows=R, k=K, g=gs):
        return dict(qweight=junk((rows, k // per), I32),
                    qzeros=junk((rows, -(-(k // g) // per)), I32),
                    scales=junk((rows, k // g), F16))

    @case
    def quantize_groups(seed):
        w = _randn((R, K), BF16, seed).to(dev)

        def call():
            o = dict(packed_outs(), tensor_q=junk(R * K, I32),
                     zeros=junk((R, G), I32))
            hip.quantize_groups(w, R, K, gs, bits, False, **o)
            return tuple(o.values())
        return [w], [], call

    @case
    def quantize_search(seed):
        w = _randn((R, K), BF16, seed).to(dev)

        def call():
            o = packed_outs()
            hip.quantize_search(w, R, K, gs, bits, False, 4, 3, **o)
            return tuple(o.values())
        return [w], [], call

    @case
    def group_params(seed):
        w = _randn((3, 200), BF16, seed).to(dev)
        return [w], [], lambda: hip.group_params(w, 3, 200, 64, bits, False)

    @case
    def apply_params(seed):
        g = torch.Generator().manual_seed(seed)
        x = torch.randint(-8, 8, (3, 200), generator=g, dtype=I32).to(dev)
        s = (torch.rand(3, 4, generator=g) * 0.01 + 1e-3).to(F16).double().to(dev)
        z = torch.randint(-8, 8, (3, 4), generator=g).double().to(dev)
        return [x, s, z], [], lambda: (hip.apply_params(x, 3, 200, 64, s, z, -8, 7, 1, F16, F16, 0),)

    @case
    def quantize_ragged(seed):
        from awq_quantizer.quantization.batch import PackedBatch
        ws = {f"w{i}": _randn(s, BF16, seed + i).to(dev) for i, s in enumerate(tb.RAGGED_SHAPES)}
        b = PackedBatch(ws, bits=bits, symmetric=False, group_size=gs)
        outs = [t for n in b.names for t in b.out[n].values()]

        def call():
            for t in outs:
                t.view(-1).view(torch.uint8).fill_(co.JUNK)
            hip.quantize_ragged(b.descs_dev, len(b.descs), b.total_tiles, bits, False,
                                torch.cuda.current_stream(dev).cuda_stream, b.block_tensor, BF16, gs, b.flags)
            return tuple(outs) + (b,)                      # (the batch stays alive with its result)
        return list(ws.values()), [b.descs_dev, b.block_tensor], call

    @case
    def stream_copy(seed):
        src = tb._words(1024, seed).to(dev)

        def call():
            dst = junk(src.shape, src.dtype)
            hip.stream_copy(src, dst, torch.cuda.current_stream(dev).cuda_stream)
            return (dst,)
        return [src], [], call

    @case
    def stream_ceiling(seed):
        src = tb._words(1024, seed).to(dev)

        def call():
            dst = junk(256, I32)
            hip.stream_ceiling(src, dst, torch.cuda.current_stream(dev).cuda_stream)
            return (dst,)
        return [src], [], call

    @case
    def dequant_ceiling(seed):
        words = tb._words(128, seed).to(dev)

        def call():
            out = junk(1024, F32)
            hip.dequant_ceiling(words, out, torch.cuda.current_stream(dev).cuda_stream)
            return (out,)
        return [words], [], call

    @case
    def export_autoawq_gemm(seed):
        N, k, g = 72, 512, 64
        qw, qz, sc = _packed_of(dev, _randn((N, k), BF16, seed), g, 4, False)

        def call():
            o = (junk((k, N // 8), I32), junk((k // g, N // 8), I32),
                 junk((k // g, N), F16))
            hip.export_autoawq_gemm(qw, qz, sc, N, k, g, 4, *o)
            return o
        return [qw, qz, sc], [], call

    @case
    def import_autoawq_gemm(seed):
        N, k, g = 72, 384, 128
        gemm, _ = imp.reference(N, k, g, bool(seed & 1))
        t = [gemm[n].to(dev) for n in ("qweight", "qzeros", "scales")]

        def call():
            o = (junk((N, k // 8), I32), junk((N, 1), I32),
                 junk((N, k // g), F16))
            hip.import_autoawq_gemm(*t, N, k, g, 4, *o)
            return o
        return t, [], call

    def quantized(seed, shape=(R, K), g=gs):
        w = _randn(shape, BF16, seed)
        e = tb.quant_expect(w, shape[0], shape[1], g, bits, False)
        return w.to(dev), {n: e[n].to(dev) for n in e}

    @case
    def dequantize(seed):
        _, e = quantized(seed)
        tq = e["tensor_q"].reshape(R, K).contiguous()

        def call():
            out = junk((R, K), F32)
            hip.dequantize(tq, e["scales"], e["zeros"], R, K, gs, out)
            return (out,)
        return [tq, e["scales"], e["zeros"]], [], call

    @case
    def dequantize_packed(seed):
        _, e = quantized(seed)

        def call():
            out = junk((R, K), F32)
            hip.dequantize_packed(e["qweight"], e["qzeros"], e["scales"], R, K, gs, bits, False, out)
            return (out,)
        return [e["qweight"], e["qzeros"], e["scales"]], [], call

    @case
    def pack_rows(seed):
        v = torch.randint(0, 16, (3, 1000), generator=torch.Generator().manual_seed(seed), dtype=I32).to(dev)

        def call():
            out = junk((3, 125), I32)
            hip.pack_rows(v, 3, 1000, 4, 0, out)
            return (out,)
        return [v], [], call

    @case
    def quant_error(seed):
        w, e = quantized(seed)
        t = [w, e["qweight"], e["qzeros"], e["scales"]]
        return t, [], lambda: hip.quant_error(w, R, K, gs, bits, False, e["qweight"], e["qzeros"], e["scales"], totals=True)

    @case
    def quant_error_no_totals(seed):
        w, e = quantized(seed, (4, 250), 100)
        t = [w, e["qweight"], e["qzeros"], e["scales"]]
        return t, [], lambda: hip.quant_error(w, 4, 250, 100, bits, False, e["qweight"], e["qzeros"], e["scales"],
                                              totals=False)[:2]

    @case
    def output_error(seed):
        w, e = quantized(seed, (40, 128), 64)
        x = _randn((33, 128), BF16, seed + 1, 1.0).to(dev)
        col = _pos(128, seed).to(dev)
        t = [w, e["qweight"], e["qzeros"], e["scales"], x, col]
        return t, [], lambda: hip.output_error(w, 64, bits, False, e["qweight"], e["qzeros"], e["scales"], x, col,
                                               ref=True, err=True)

    @case
    def act_stats(seed):
        x = _randn((257, 264), BF16, seed, 3.0).to(dev)
        return [x], [], lambda: hip.act_stats(x)

    def accs(k, seed):
        sa, sq = _seeds(k)
        return (sa + seed).to(dev), (sq + seed).to(dev)

    @case
    def act_stats_accum(seed):
        x = _randn((CALIB_T, 8), BF16, seed, 2.0).to(dev)
        a, q = accs(8, seed)

        def call():
            hip.act_stats_accum(x, 0, a, q)
            return a, q
        return [x, a, q], [], call

    @case
    def rmsnorm_stats(seed):
        x = _randn((CALIB_T, 8), BF16, seed, 1.5).to(dev)
        w = (1 + _randn((8,), F32, seed + 1, 0.2)).to(BF16).to(dev)
        a, q = accs(8, seed)
        return [x, w, a, q], [], lambda: (hip.rmsnorm_stats(x, w, 1e-5, 0, a, q), a, q)

    @case
    def swiglu_stats(seed):
        g = _randn((CALIB_T, 8), BF16, seed, 4.0).to(dev)
        u = _randn((CALIB_T, 8), BF16, seed + 1, 1.0).to(dev)
        a, q = accs(8, seed)
        return [g, u, a, q], [], lambda: (hip.swiglu_stats(g, u, 0, a, q), a, q)

    @case
    def column_mean(seed):
        a, _ = accs(264, seed)
        return [a], [], lambda: (hip.column_mean(a, 7.0),)

    @case
    def weight_mean(seed):
        ws = [_randn((r, 256), BF16, seed + r, 0.05).to(dev) for r in (1, 257)]
        return ws, [], lambda: (hip.weight_mean(ws, 16), hip.weight_mean(ws, 128))

    @case
    def act_scale_table(seed):
        xm, wm = _pos(264, seed).to(dev), _pos(264, seed + 1).to(dev)
        return [xm, wm], [], lambda: (hip.act_scale_table(xm, wm, 5), hip.act_scale_table(xm, wm, 5, workspace=False))

    @case
    def act_recip_table(seed):
        t = _pos(5 * 264, seed).reshape(5, 264).to(dev)
        return [t], [], lambda: (hip.act_recip_table(t),)

    @case
    def act_search_losses(seed):
        ws = [_randn((r, 256), BF16, seed + r, 0.02).to(dev) for r in (3, 5)]
        xs = (_pos(256, seed) ** 2).to(dev)
        table = _pos(5 * 256, seed + 1).reshape(5, 256).to(dev)
        rt = (torch.ones((), dtype=F32) / table.cpu()).to(dev)
        return ws + [xs, table, rt], [], lambda: (hip.act_search_losses(ws, xs, table, 128, bits, False, rtable=rt),
                                                  hip.act_search_losses(ws, xs, table, 128, bits, False, use_rtable=False))

    @case
    def act_search_select(seed):
        part = _pos(5 * 1025, seed).reshape(5, 1025).to(dev)
        table = _pos(5 * 24, seed + 1).reshape(5, 24).to(dev)
        return [part, table], [], lambda: hip.act_search_select(part, table)

    @case
    def quantize_groups_scaled(seed):
        w, s = _randn((23, 384), BF16, seed).to(dev), _pos(384, seed).to(dev)

        def call():
            o = packed_outs(23, 384)
            hip.quantize_groups_scaled(w, s, gs, bits, False, **o)
            return tuple(o.values())
        return [w, s], [], call

    def clip_outs(rows, k, g, nc=0):
        n = rows * (k // g)
        o = dict(packed_outs(rows, k, g), best_idx=junk(n, I32),
                 group_loss=junk((2, n), F32))
        if nc:
            o["cand_loss"] = junk((nc, n), F32)
        return o

    @case
    def quantize_clip_scaled(seed):
        w, s = _randn((23, 384), BF16, seed).to(dev), _pos(384, seed).to(dev)
        xs = (_pos(384, seed + 1) ** 2).to(dev)
        rs = (torch.ones((), dtype=F32) / s.cpu()).to(dev)

        def call():
            o = clip_outs(23, 384, gs)
            hip.quantize_clip_scaled(w, s, xs, gs, bits, False, 20, 10, rscale=rs, **o)
            return tuple(o.values())
        return [w, s, xs, rs], [], call

    @case
    def quantize_clip_output(seed):
        w, s = _randn((33, 384), BF16, seed).to(dev), _pos(384, seed).to(dev)
        x = _randn((33, 384), BF16, seed + 1, 1.0).to(dev)
        rs = (torch.ones((), dtype=F32) / s.cpu()).to(dev)

        def call():
            o = clip_outs(33, 384, gs, 10)
            hip.quantize_clip_output(w, s, x, gs, bits, False, 20, 10, rscale=rs, **o)
            return tuple(o.values())
        return [w, s, x, rs], [], call

    @case
    def apply_input_scale(seed):
        w, s = _randn((3, 264), BF16, seed).to(dev), _pos(264, seed).to(dev)
        return [w, s], [], lambda: (hip.apply_input_scale(w, s),)

    @case
    def fold_rows(seed):
        w, s = _randn((5, 264), BF16, seed).to(dev), _pos(5, seed).to(dev)
        v = _randn((13,), BF16, seed + 1).to(dev)
        sv = _pos(13, seed + 1).to(dev)
        return [w, s, v, sv], [], lambda: (hip.fold_rows(w, s), hip.fold_rows(v, sv))

    return cases


# Wrappers that block the host before they return cannot meet step 4 (stream 0 synchronised while
# the gate still spins): their result is only compared.
BLOCKING = {
    "quant_error": "with totals the caller reads the five fp64 totals back at once (quantization_error does); the "
                   "case makes that readback part of the call",
    "selftest": "returns the mismatch count as a Python int: a device-to-host copy inside the wrapper",
}


def _host(result):
    return [None if t is None else tb._bytes(t) for t in result if t is None or isinstance(t, torch.Tensor)]


def test_order_wrappers():
    """Every launching wrapper from quantize_groups to fold_rows: the result on the default stream,
    a decoy call on other data (so that memory the allocator hands out again does not hold the
    answer), then the same call behind the gate on stale inputs — bit for bit the first result."""
    dev = _dev()
    from awq_quantizer import _hip
    cases = wrapper_cases(_hip, dev)
    launching = {"quantize_groups", "quantize_search", "group_params", "apply_params", "quantize_ragged", "stream_copy",
                 "stream_ceiling", "dequant_ceiling", "export_autoawq_gemm", "import_autoawq_gemm", "dequantize",
                 "dequantize_packed", "pack_rows", "quant_error", "output_error", "act_stats", "act_stats_accum",
                 "rmsnorm_stats", "swiglu_stats", "column_mean", "weight_mean", "act_scale_table", "act_recip_table",
                 "act_search_losses", "act_search_select", "quantize_groups_scaled", "quantize_clip_scaled",
                 "quantize_clip_output", "apply_input_scale", "fold_rows"}
    assert launching <= set(cases), sorted(launching - set(cases))
    failed = []

    def blocking(name, call):
        if name != "quant_error":
            return call
        def with_readback():
            r = call()
            return r + (r[2].cpu(),)
        return with_readback

    want = {}
    for name, make in cases.items():
        for seed in (11, 12):                                   # 12: the decoy
            _, _, call = make(seed)
            r = _host(blocking(name, call)())
            torch.cuda.synchronize(dev)
            if seed == 11:
                want[name] = r
    want["selftest"] = _hip.selftest(0, dev)
    with stream_gate.ordered(dev) as st:
        for name, make in cases.items():
            st.case = f"_hip.{name}"
            tensors, pointers, call = make(11)
            got = stream_gate.run_tensors(st, tensors, blocking(name, call), pointers=[p for p in pointers if p is not None],
                                          blocks=name in BLOCKING)
            got = _host(got)
            if len(got) != len(want[name]) or not all((a is None and b is None) or torch.equal(a, b)
                                                      for a, b in zip(got, want[name])):
                failed.append(st.case)
        st.case = "_hip.selftest"
        assert st.behind_gate(lambda: None, lambda: _hip.selftest(0, dev), blocks=True) == want["selftest"] == 0
        ms, where = st.longest_span_ms()
        print(f"{st.gates} gates; longest span {ms:.3f} ms ({where})")
    assert not failed, f"differ from their default-stream result: {failed}"


# ---------------------------------------------------------------- 3. the class API
def _flat(r, prefix=""):
    """Every tensor of a nested result, by path; other leaves as they are."""
    if isinstance(r, dict):
        out = {}
        for k, v in r.items():
            out.update(_flat(v, f"{prefix}/{k}"))
        return out
    if isinstance(r, (list, tuple)):
        out = {}
        for i, v in enumerate(r):
            out.update(_flat(v, f"{prefix}/{i}"))
        return out
    if isinstance(r, torch.Tensor):
        return {prefix: tb._bytes(r)}
    return {prefix: r}


def _same(fa, fb):
    """Two _flat() results: None if equal, else what differs."""
    if set(fa) != set(fb):
        return f"keys differ: {sorted(set(fa) ^ set(fb))}"
    for k in fa:
        x, y = fa[k], fb[k]
        if isinstance(x, torch.Tensor):
            if not (isinstance(y, torch.Tensor) and torch.equal(x, y)):
                return k
        elif not (x == y or (x != x and y != y)):
            return k
    return None


def api_calls(dev):
    from awq_quantizer.quantization import AWQQuantizer, act_search

    def q(gs, **kw):
        return AWQQuantizer(**dict(dict(bits=4, group_size=gs, symmetric=False, device="cuda:0", logger_level="ERROR"), **kw))

    calls = {}
    for name, shape, dtype, gs in (("streaming", (3, 1024), BF16, 128), ("padded rows", (5, 200), BF16, 128),
                                   ("row segment", (4, 250), BF16, 100), ("generic fp64", (3, 200), F64, 64),
                                   ("generic gs 1024", (2, 2088), BF16, 1024)):
        calls[f"quantize_packed {name}"] = lambda s=shape, d=dtype, g=gs: q(g).quantize_packed(_randn(s, d, 5))
    calls["dequantize_packed"] = lambda: q(128).dequantize_packed(q(128).quantize_packed(_randn((3, 1024), BF16, 5)))
    model = {"a": _randn((3, 1024), BF16, 1), "b": _randn((23, 384), BF16, 2), "c": _randn((5, 200), BF16, 3),
             "bias": _randn((256,), BF16, 4), "d": _randn((3, 200), F64, 5)}

    def model_packed():
        r = q(128).quantize_model_packed(model)
        assert list(r) == list(model)
        return r
    calls["quantize_model_packed"] = model_packed

    def round_trip():
        qq = q(64)
        g = qq.export_autoawq(qq.quantize_packed(_randn((72, 512), BF16, 6)))
        return g, qq.import_autoawq(g)
    calls["export_autoawq, import_autoawq"] = round_trip
    ws, x = co._api_inputs()
    qa = lambda: co._quantizer()
    calls["quantize_layer_group diag"] = lambda: qa().quantize_layer_group(ws, x)
    calls["quantize_layer_group clip"] = lambda: qa().quantize_layer_group(ws, x, clip=True)
    calls["quantize_layer_group clip_loss=output"] = lambda: act_search.quantize_layer_group(
        qa(), ws, x, clip=True, clip_loss="output", samples=x)
    return calls


def test_order_class_api():
    """The class API under ordered(): bit for bit its default-stream results (PackedBatch's tables
    go up on S); then a PackedBatch built on the default stream and run(stream=S) behind the gate
    (the `_ready` event of batch.py), batch and outputs alive until S has synchronised."""
    dev = _dev()
    from awq_quantizer.quantization.batch import PackedBatch
    calls = api_calls(dev)
    want = {}
    for name, call in calls.items():
        want[name] = _flat(call())
        torch.cuda.synchronize(dev)
    failed = []
    ws = {f"w{i}": _randn(s, BF16, 20 + i).to(dev) for i, s in enumerate(tb.RAGGED_SHAPES)}
    ref = PackedBatch(ws, bits=4, group_size=128)
    ref.run()
    torch.cuda.synchronize(dev)
    ref = _flat(ref.results())
    batch = PackedBatch(ws, bits=4, group_size=128)              # tables on the default stream
    for o in batch.out.values():
        for t in o.values():
            t.view(-1).view(torch.uint8).fill_(0x5A)
    torch.cuda.synchronize(dev)
    with stream_gate.ordered(dev) as st:
        for name, call in calls.items():
            st.case = name
            got = call()
            st.stream.synchronize()
            bad = _same(_flat(got), want[name])
            if bad:
                failed.append(f"{name}: {bad}")
        st.case = "PackedBatch.run(stream=S)"
        assert batch._stream0 != st.stream
        stream_gate.run_tensors(st, list(ws.values()), lambda: batch.run(stream=st.stream),
                                pointers=[batch.descs_dev, batch.block_tensor])
        bad = _same(_flat(batch.results()), ref)
        if bad:
            failed.append(f"{st.case}: {bad}")
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------- 4. two threads, two streams
def test_two_threads_two_streams():
    """Two host threads, each with its own stream and buffers, 50 rounds over four multi-launch
    entries (quant_error with totals, output_error, quantize_clip_output, act_stats) on different
    shapes, started behind a barrier; ctypes drops the GIL, so the entries' host code overlaps.
    Every result equals, bit for bit, the same call made serially.  This test can only ever fail
    for a real bug (shared host state, a launch on another stream): a pass is weaker evidence than
    the ordered cases above, which make a misplaced launch fail deterministically."""
    dev = _dev()
    from awq_quantizer import _hip
    cases = wrapper_cases(_hip, dev)
    names = ("quant_error", "output_error", "quantize_clip_output", "act_stats")
    ROUNDS, TIMEOUT = 50, 120.0
    plans = []
    for t in range(2):
        calls, want = [], []
        for name in names:
            _, _, call = cases[name](30 + 7 * t)
            calls.append(call)
            want.append(_host(call()))
        plans.append((calls, want))
    torch.cuda.synchronize(dev)
    barrier = threading.Barrier(2)
    errors, rounds = [None, None], [0, 0]

    def work(t):
        try:
            calls, want = plans[t]
            s = torch.cuda.Stream(dev)
            barrier.wait(TIMEOUT)
            with torch.cuda.stream(s):
                for r in range(ROUNDS):
                    results = [call() for call in calls]
                    s.synchronize()
                    for name, got, w in zip(names, results, want):
                        got = _host(got)
                        if not all(torch.equal(a, b) for a, b in zip(got, w)):
                            raise AssertionError(f"thread {t} round {r}: {name} differs from the serial call")
                    rounds[t] += 1
        except BaseException as e:          # reported by the main thread
            errors[t] = e
            barrier.abort()

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(TIMEOUT)
    assert not any(th.is_alive() for th in threads), "a thread did not finish in time"
    for e in errors:
        if e is not None:
            raise e
    assert rounds == [ROUNDS, ROUNDS]
