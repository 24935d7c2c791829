#!/usr/bin/env python3
"""awq_quant_error (the fused quantization-error report) against the two things it is quoted
against, interleaved in one process on the same tensors (HIP events, `--rounds` rounds of
windows of at least `--window-ms` each, medians; every case cycles over enough copies of the
tensor that no launch finds its input in the Infinity Cache):
  * composed: the path available without it — dequantize_packed into fp32, then torch for
    w - dq, |d|, d^2, w^2 and their sums;
  * rtn: the awq_quantize_groups call that made the packed result (a stream of similar size:
    it reads the same weights and writes what the report reads).
Default shapes: Llama-3-8B's MLP down / up projections and lm_head, bf16, gs 128, 4-bit.
One JSON line per shape: microseconds, algorithmic bytes, fraction of 8 TB/s, the ratios.

  python scripts/qerror_bench.py [--shapes 14336x4096,4096x14336,128256x4096]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "awq-converter_amd")]
import torch  # noqa: E402

from awq_quantizer import _hip  # noqa: E402
from awq_quantizer.quantization import AWQQuantizer  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def bench_shape(rows, K, L, bits, rounds, window_ms, footprint):
    """Every case cycles over `reps` copies of the tensor and its packed result, enough that one
    cycle's weights exceed `footprint` bytes (past the 256 MiB Infinity Cache: a launch never finds
    its input left there by the launch before), and every timed window holds enough launches to
    last `window_ms` (so the clock and the scheduler do not dominate a 50 us kernel)."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(rows + K)
    q = AWQQuantizer(bits=bits, group_size=L, symmetric=False, device="cuda:0", logger_level="ERROR")
    n, G = rows * K, K // L
    ng = rows * G
    reps = max(1, -(-footprint // (n * 2)))
    xs = [(torch.randn(rows, K, device=dev, generator=g) * 0.02).bfloat16() for _ in range(reps)]
    ps = [q.quantize_packed(x) for x in xs]
    lib = _hip.load_library()
    stats = torch.empty((4, ng), dtype=torch.float32, device=dev)
    bad = torch.empty(ng, dtype=torch.int32, device=dev)
    work = torch.empty(lib.awq_quant_error_work_bytes(rows, K, L) // 8, dtype=torch.float64, device=dev)
    tot = torch.empty(5, dtype=torch.float64, device=dev)
    dq = torch.empty((rows, K), dtype=torch.float32, device=dev)
    stream = _hip._stream(xs[0])
    out = q._packed_outputs(xs[0])
    turn = {"i": 0}

    def pick():
        turn["i"] = (turn["i"] + 1) % reps
        return xs[turn["i"]], ps[turn["i"]]

    def call(x, p, with_totals):
        _hip.check(lib.awq_quant_error(_hip.ptr(x), 0, rows, K, L, bits, 0, _hip.ptr(p["qweight"]),
                                       _hip.ptr(p["qzeros"]), _hip.ptr(p["scales"]), _hip.ptr(stats), _hip.ptr(bad),
                                       _hip.ptr(work) if with_totals else None,
                                       _hip.ptr(tot) if with_totals else None, stream), "awq_quant_error")

    def fused():
        call(*pick(), True)

    def fused_level1():
        call(*pick(), False)

    keep = {}

    def composed():
        x, p = pick()
        _hip.dequantize_packed(p["qweight"], p["qzeros"], p["scales"], rows, K, L, bits, False, dq)
        d = x - dq
        keep["r"] = (d.abs().sum(), d.square().sum(), x.float().square().sum())

    def rtn():
        x, _ = pick()
        _hip.quantize_groups(x, rows, K, L, bits, False, qweight=out["qweight"], qzeros=out["qzeros"],
                             scales=out["scales"])

    cases = {"fused": fused, "fused_level1": fused_level1, "composed": composed, "rtn": rtn}
    iters = {}
    for name, fn in cases.items():          # warm-up of every case on this shape, and its window length
        fn()
        torch.cuda.synchronize()
        iters[name] = max(10, int(window_ms * 1e3 / max(timed(fn, 10), 1.0)) + 1)
    turn["i"] = reps - 1                    # both on copy 0: the two paths' sums side by side
    fused()
    turn["i"] = reps - 1
    composed()
    torch.cuda.synchronize()
    agree = [float(v) for v in tot.tolist()[:3]], [float(v) for v in keep["r"]]
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for name, fn in cases.items():
            times[name].append(timed(fn, iters[name]))
    us = {k: statistics.median(v) for k, v in times.items()}
    par = ng * 2 + rows * -(-G * bits // 32) * 4                   # scales + qzeros
    alg_fused = n * 2 + n * bits // 8 + par + ng * 20              # reads w, qweight, parameters; writes level 1
    alg_rtn = n * 2 + n * bits // 8 + par                          # reads w; writes qweight, parameters
    rate = {"fused": alg_fused / us["fused"] / 1e6, "level1": alg_fused / us["fused_level1"] / 1e6,
            "rtn": alg_rtn / us["rtn"] / 1e6}
    return {"rows": rows, "K": K, "group_size": L, "bits": bits, "dtype": "bf16", "tensor_copies_cycled": reps,
            "launches_per_window": iters,
            "fused_us": round(us["fused"], 1), "fused_level1_us": round(us["fused_level1"], 1),
            "composed_us": round(us["composed"], 1), "rtn_us": round(us["rtn"], 1),
            "fused_us_min_max": [round(min(times["fused"]), 1), round(max(times["fused"]), 1)],
            "fused_level1_us_min_max": [round(min(times["fused_level1"]), 1), round(max(times["fused_level1"]), 1)],
            "composed_us_min_max": [round(min(times["composed"]), 1), round(max(times["composed"]), 1)],
            "rtn_us_min_max": [round(min(times["rtn"]), 1), round(max(times["rtn"]), 1)],
            "fused_algorithmic_bytes": alg_fused, "rtn_algorithmic_bytes": alg_rtn,
            "fused_TBs": round(rate["fused"], 3), "fused_frac_8TBs": round(rate["fused"] / 8, 4),
            "level1_TBs": round(rate["level1"], 3), "level1_frac_8TBs": round(rate["level1"] / 8, 4),
            "rtn_TBs": round(rate["rtn"], 3), "rtn_frac_8TBs": round(rate["rtn"] / 8, 4),
            "speedup_over_composed": round(us["composed"] / us["fused"], 2),
            "rate_over_rtn_rate": round(rate["fused"] / rate["rtn"], 3),
            "level1_rate_over_rtn_rate": round(rate["level1"] / rate["rtn"], 3),
            "sums_fused_vs_composed": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="14336x4096,4096x14336,128256x4096")
    ap.add_argument("--group-size", type=int, default=128)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0, help="least length of a timed window")
    ap.add_argument("--footprint-mib", type=int, default=1024,
                    help="weights cycled through before a tensor is read again (0: one copy, cache-warm)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qerror_bench: needs a GPU (no CPU fallback; a CPU timing would say nothing)")
    _hip.require_device(torch.device("cuda", 0))
    for s in a.shapes.split(","):
        rows, K = (int(v) for v in s.lower().split("x"))
        r = bench_shape(rows, K, a.group_size, a.bits, a.rounds, a.window_ms, a.footprint_mib << 20)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
