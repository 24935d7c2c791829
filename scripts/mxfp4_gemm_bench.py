#!/usr/bin/env python3
"""awq_mxfp4_gemm against what evaluate did before it — awq_dequantize_mxfp4 of both
operands to bf16 followed by torch.matmul — and against that bf16 matmul alone, on the same operands, every
case into preallocated buffers, interleaved in one process (HIP events, `--rounds` rounds of windows of at
least `--window-ms` each, medians with the spread).  One JSON line per shape: microseconds, TFLOP/s
(2 T N K per call) and the kernel's rate over the two others'.

  python scripts/mxfp4_gemm_bench.py [--shapes 8192x4096x4096,8192x14336x4096,8192x4096x14336,512x4096x4096]
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
from mxfp4_bench import timed  # noqa: E402


def operand(rows, K, dev, g):
    x = (torch.randn(rows, K, device=dev, generator=g) * 0.02).bfloat16()
    codes = torch.empty((rows, K // 2), dtype=torch.uint8, device=dev)
    scales = torch.empty((rows, K // 32), dtype=torch.uint8, device=dev)
    _hip.quantize_mxfp4(x, "floor", codes, scales)
    return codes, scales, torch.empty_like(x)


def bench_shape(T, N, K, rounds, window_ms):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(T + N + K)
    (ac, asc, a16), (wc, ws, w16) = operand(T, K, dev, g), operand(N, K, dev, g)
    out = torch.empty((T, N), dtype=torch.bfloat16, device=dev)
    w16t = w16.t()

    def dequant_matmul():
        _hip.dequantize_mxfp4(ac, asc, a16)
        _hip.dequantize_mxfp4(wc, ws, w16)
        torch.matmul(a16, w16t, out=out)

    cases = {"mxfp4_gemm": lambda: _hip.mxfp4_gemm(ac, asc, wc, ws, out),
             "dequant_bf16_matmul": dequant_matmul,
             "bf16_matmul": lambda: torch.matmul(a16, w16t, out=out)}
    iters = {}
    for name, fn in cases.items():     # warm-up of every case on this shape, and its window length
        fn()
        torch.cuda.synchronize()
        iters[name] = max(3, int(window_ms * 1e3 / max(timed(fn, 3), 1.0)) + 1)
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for name, fn in cases.items():
            times[name].append(timed(fn, iters[name]))
    us = {k: statistics.median(v) for k, v in times.items()}
    r = {"device": torch.cuda.get_device_name(0), "T": T, "N": N, "K": K, "out": "bf16"}
    for k in cases:
        r[k + "_us"] = round(us[k], 1)
        r[k + "_us_min_max"] = [round(min(times[k]), 1), round(max(times[k]), 1)]
        r[k + "_TFLOPs"] = round(2.0 * T * N * K / us[k] * 1e-6, 1)
    r["gemm_over_dequant_matmul"] = round(us["dequant_bf16_matmul"] / us["mxfp4_gemm"], 3)
    r["gemm_over_bf16_matmul"] = round(us["bf16_matmul"] / us["mxfp4_gemm"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x4096x4096,8192x14336x4096,8192x4096x14336,512x4096x4096", help="TxNxK,...")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0, help="least length of a timed window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_gemm_bench: needs a GPU (no CPU fallback; a CPU timing would say nothing)")
    _hip.require_device(torch.device("cuda", 0))
    for sh in a.shapes.split(","):
        T, N, K = (int(v) for v in sh.lower().split("x"))
        print(json.dumps(bench_shape(T, N, K, a.rounds, a.window_ms)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
