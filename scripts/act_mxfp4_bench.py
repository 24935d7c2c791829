#!/usr/bin/env python3
"""The activation-aware MXFP4 kernels (csrc/awq_act_mxfp4.hip) in one process, alternating on
the same buffers, window by window: awq_act_search_losses_mxfp4 against awq_act_search_losses at group size
32 (4 bits, asymmetric) on the same weights, table and reciprocals; awq_quantize_mxfp4_scaled against
awq_apply_input_scale + awq_quantize_mxfp4 and against awq_stream_copy of the weight.  bf16, --grid
candidates, rules floor and mse.  Medians of --windows windows of --reps launches between two events, with
the spread (max - min) / median.  One JSON line per shape and rule.

    python scripts/act_mxfp4_bench.py [--windows 9] [--reps 5] [--grid 20] [--shapes 4096x4096,14336x4096,4096x14336]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "awq-converter_amd"))
from awq_quantizer import _hip  # noqa: E402


def alternate(fns, n_windows, reps):
    """name -> (median ms per launch, spread): every window times each function in turn."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(n_windows):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / reps)
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--shapes", default="4096x4096,14336x4096,4096x14336")
    args = ap.parse_args()
    if args.windows < 7:
        sys.exit("--windows must be at least 7")
    dev = torch.device("cuda")
    _hip.require_device(dev)
    lib, P = _hip.load_library(), _hip.ptr
    for shape in args.shapes.split(","):
        N, K = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(N + K)
        w = (torch.randn(N, K, generator=g) * 0.02).bfloat16().to(dev)
        x_mean = (torch.rand(K, generator=g) * 4 + 0.01).to(dev)
        x_sq = (torch.rand(K, generator=g) * 3 + 0.1).to(dev)
        table = _hip.act_scale_table(x_mean, _hip.weight_mean([w], 32), args.grid)
        rtable = _hip.act_recip_table(table)
        s = table[args.grid // 2].contiguous()
        nblk = N * K // 32
        part = torch.empty((args.grid, nblk), dtype=torch.float32, device=dev)
        copy = torch.empty_like(w)
        codes = torch.empty((N, K // 2), dtype=torch.uint8, device=dev)
        scales = torch.empty((N, K // 32), dtype=torch.uint8, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for rule, rc in (("floor", 0), ("mse", 2)):
            fns = {
                "loss_int4_gs32": lambda: _hip.check(lib.awq_act_search_losses(
                    P(w), 0, N, K, 32, 4, 0, P(table), P(rtable), args.grid, P(x_sq), P(part), nblk, st), "int loss"),
                "loss_mxfp4": lambda: _hip.check(lib.awq_act_search_losses_mxfp4(
                    P(w), 0, N, K, rc, P(table), P(rtable), args.grid, P(x_sq), P(part), nblk, st), "mxfp4 loss"),
                "quantize_scaled": lambda: _hip.check(lib.awq_quantize_mxfp4_scaled(
                    P(w), 0, N, K, rc, P(s), P(codes), P(scales), st), "scaled"),
                "apply_then_quantize": lambda: (
                    _hip.check(lib.awq_apply_input_scale(P(w), 0, N, K, P(s), P(copy), st), "apply"),
                    _hip.check(lib.awq_quantize_mxfp4(P(copy), 0, N, K, rc, P(codes), P(scales), st), "quantize")),
                "quantize_plain": lambda: _hip.check(lib.awq_quantize_mxfp4(
                    P(w), 0, N, K, rc, P(codes), P(scales), st), "quantize"),
                "stream_copy": lambda: _hip.check(lib.awq_stream_copy(P(w), P(copy), w.numel() * 2, st), "copy"),
            }
            r = alternate(fns, args.windows, args.reps)
            row = {"shape": shape, "rule": rule, "grid": args.grid, "windows": args.windows, "reps": args.reps}
            for k, (med, spread) in r.items():
                row[k + "_ms"], row[k + "_spread"] = round(med, 4), round(spread, 4)
            ce = N * K * args.grid
            row["loss_int4_ps_per_cand_elem"] = round(r["loss_int4_gs32"][0] * 1e9 / ce, 3)
            row["loss_mxfp4_ps_per_cand_elem"] = round(r["loss_mxfp4"][0] * 1e9 / ce, 3)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
