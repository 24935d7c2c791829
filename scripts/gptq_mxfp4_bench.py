#!/usr/bin/env python3
"""awq_gptq_round_block_mxfp4 (csrc/awq_gptq_round_mxfp4.hip) against awq_gptq_round_block at
group size 32, 4 bits, asymmetric — the integer solver on the same block — in one process, alternating
on the same work / U buffers: one 128-column call, the whole solve (the calls plus the trailing torch
GEMMs), and quantize_gptq_mxfp4 against quantize_gptq end to end.  Medians of --windows windows of
--reps launches between two events, with the spread (max - min) / median.  One JSON line per row.

    python scripts/gptq_mxfp4_bench.py [--windows 9] [--reps 20] [--shapes 4096x4096,14336x4096,4096x14336]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "awq-converter_amd"))
from awq_quantizer import _hip  # noqa: E402
from awq_quantizer.quantization import AWQQuantizer  # noqa: E402


def windows(fn, n_windows, reps):
    """ms per launch: the median over the windows and their spread."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    med = statistics.median(ms)
    return med, (max(ms) - min(ms)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="4096x4096,14336x4096,4096x14336")
    ap.add_argument("--tokens", type=int, default=512)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    for shape in args.shapes.split(","):
        N, K = (int(v) for v in shape.split("x"))
        w0 = (torch.randn(N, K, generator=g) * 0.05).to(dev)
        U = torch.triu(torch.randn(K, K, generator=g) * 0.01).to(dev)
        U.diagonal().copy_(torch.rand(K, generator=g) + 0.5)
        U = U.contiguous()
        work = w0.clone()
        err = torch.empty((N, 128), dtype=torch.float32, device=dev)
        codes = torch.empty((N, K // 2), dtype=torch.uint8, device=dev)
        sb = torch.empty((N, K // 32), dtype=torch.uint8, device=dev)
        qw = torch.empty((N, K // 8), dtype=torch.int32, device=dev)
        qz = torch.zeros((N, (K // 32 + 7) // 8), dtype=torch.int32, device=dev)
        sc = torch.empty((N, K // 32), dtype=torch.float16, device=dev)

        def call_int4(c0=0):
            _hip.gptq_round_block(work, U, 32, 4, False, c0, 128, err, qw, qz, sc)

        def call_mx(rule, c0=0):
            _hip.gptq_round_block_mxfp4(work, U, rule, c0, 128, err, codes, sb)

        def solve(call):
            work.copy_(w0)
            for c0 in range(0, K, 128):
                call(c0)
                if c0 + 128 < K:
                    work[:, c0 + 128:].addmm_(err, U[c0:c0 + 128, c0 + 128:], alpha=-1.0)

        rows = {}
        for _ in range(2):          # alternating: int4, floor, mse, twice; the later pass is reported
            work.copy_(w0)
            rows["call int4 g32"] = windows(call_int4, args.windows, args.reps)
            for rule in ("floor", "mse"):
                work.copy_(w0)
                rows[f"call mxfp4 {rule}"] = windows(lambda: call_mx(rule), args.windows, args.reps)
            rows["solve int4 g32"] = windows(lambda: solve(call_int4), args.windows, 2)
            for rule in ("floor", "mse"):
                rows[f"solve mxfp4 {rule}"] = windows(lambda: solve(lambda c0: call_mx(rule, c0)), args.windows, 2)
        for name, (med, spread) in rows.items():
            print(json.dumps({"shape": shape, "what": name, "ms": round(med, 4), "spread": round(spread, 4)}), flush=True)
        del work, w0, codes, sb, qw, qz, sc, err

        if shape == args.shapes.split(",")[0]:     # end to end, the first shape
            w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(dev)
            x = torch.randn(args.tokens, K, generator=g).to(torch.bfloat16).to(dev)
            q = AWQQuantizer(bits=4, group_size=32, symmetric=False, device="cuda:0", logger_level="ERROR")
            for name, fn in (("quantize_gptq g32", lambda: q.quantize_gptq(w, x)),
                             ("quantize_gptq_mxfp4 floor", lambda: q.quantize_gptq_mxfp4(w, x))):
                med, spread = windows(fn, max(args.windows, 7), 1)
                print(json.dumps({"shape": shape, "what": name, "tokens": args.tokens, "ms": round(med, 3),
                                  "spread": round(spread, 4)}), flush=True)
        del U
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
