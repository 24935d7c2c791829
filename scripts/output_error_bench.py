#!/usr/bin/env python3
"""awq_output_error (the output-space error on token samples) against the two things it is quoted
against, interleaved in one process on the same tensors (HIP events, `--rounds` rounds of windows
of at least `--window-ms` each, medians and min / max; every case cycles over enough copies of the
weights that no launch finds them in the Infinity Cache):
  * composed: the path available without it — dequantize_packed into fp32, divide by col_scale,
    subtract the fp32 weights, one fp32 torch.matmul with X^T, square, sum over tokens (and the
    same product for W X^T when ref_sq is asked for);
  * bf16_matmul: one bf16 torch.matmul of the same (N, K, T): the library's rate for ONE MFMA per
    k-step; the fused kernel issues two (three with ref_sq), so its work is quoted as a fraction
    of twice (three times) that rate's FLOPs.
Default shapes: Llama-3-8B's MLP up / down projections and lm_head, bf16, gs 128, 4-bit, T = 512,
with col_scale.  One JSON line per shape, and `--search-block` adds the per-block cost of the
scale search with loss="output" (20 candidates) beside the diagonal search's.

  python scripts/output_error_bench.py [--shapes 14336x4096,4096x14336,128256x4096] [--tokens 512]
"""
import argparse
import json
import os
import statistics
import sys
import time

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


def bench_shape(N, K, T, L, bits, rounds, window_ms, footprint):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(N + K)
    q = AWQQuantizer(bits=bits, group_size=L, symmetric=False, device="cuda:0", logger_level="ERROR")
    reps = max(1, -(-footprint // (N * K * 2)))
    ws = [(torch.randn(N, K, device=dev, generator=g) * 0.02).bfloat16() for _ in range(reps)]
    ps = [q.quantize_packed(w) for w in ws]
    x = torch.randn(T, K, device=dev, generator=g).bfloat16()
    x32t = x.float().t().contiguous()
    col = torch.exp((torch.rand(K, device=dev, generator=g) * 2 - 1) * 1.386).float()
    lib = _hip.load_library()
    work = torch.empty(lib.awq_output_error_work_bytes(N, T) // 4, dtype=torch.float32, device=dev)
    e_sq = torch.empty(N, dtype=torch.float32, device=dev)
    r_sq = torch.empty(N, dtype=torch.float32, device=dev)
    dq = torch.empty((N, K), dtype=torch.float32, device=dev)
    stream = _hip._stream(x)
    turn = {"i": 0}
    keep = {}

    def pick():
        turn["i"] = (turn["i"] + 1) % reps
        return ws[turn["i"]], ps[turn["i"]]

    def call(w, p, ref):
        _hip.check(lib.awq_output_error(_hip.ptr(w), 0, N, K, L, bits, 0, _hip.ptr(p["qweight"]), _hip.ptr(p["qzeros"]),
                                        _hip.ptr(p["scales"]), _hip.ptr(col), _hip.ptr(x), T, K, _hip.ptr(work),
                                        _hip.ptr(e_sq), _hip.ptr(r_sq) if ref else None, None, stream),
                   "awq_output_error")

    def fused():
        call(*pick(), False)

    def fused_ref():
        call(*pick(), True)

    def composed_of(ref):
        def run():
            w, p = pick()
            _hip.dequantize_packed(p["qweight"], p["qzeros"], p["scales"], N, K, L, bits, False, dq)
            w32 = w.float()
            d = dq / col - w32
            keep["e"] = torch.matmul(d, x32t).square().sum(dim=1)
            if ref:
                keep["r"] = torch.matmul(w32, x32t).square().sum(dim=1)
        return run

    def bf16_matmul():
        w, _ = pick()
        keep["m"] = torch.matmul(w, x.t())

    cases = {"fused": fused, "fused_ref": fused_ref, "composed": composed_of(False), "composed_ref": composed_of(True),
             "bf16_matmul": bf16_matmul}
    iters = {}
    for name, fn in cases.items():          # warm-up of every case on this shape, and its window length
        fn()
        torch.cuda.synchronize()
        iters[name] = max(3, int(window_ms * 1e3 / max(timed(fn, 3), 1.0)) + 1)
    turn["i"] = reps - 1                    # both on copy 0: the two paths' sums side by side
    fused_ref()
    turn["i"] = reps - 1
    cases["composed_ref"]()
    torch.cuda.synchronize()
    agree = {"err_sq": [float(e_sq.double().sum()), float(keep["e"].double().sum())],
             "ref_sq": [float(r_sq.double().sum()), float(keep["r"].double().sum())]}
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for name, fn in cases.items():
            times[name].append(timed(fn, iters[name]))
    us = {k: statistics.median(v) for k, v in times.items()}
    flop = 2.0 * N * K * T
    lib_rate = flop / us["bf16_matmul"] / 1e6          # TFLOP/s of one MFMA per k-step
    out = {"N": N, "K": K, "T": T, "group_size": L, "bits": bits, "dtype": "bf16", "weight_copies_cycled": reps,
           "launches_per_window": iters}
    for k in cases:
        out[k + "_us"] = round(us[k], 1)
        out[k + "_us_min_max"] = [round(min(times[k]), 1), round(max(times[k]), 1)]
    out.update(speedup_over_composed=round(us["composed"] / us["fused"], 2),
               speedup_over_composed_ref=round(us["composed_ref"] / us["fused_ref"], 2),
               bf16_matmul_TFLOPs=round(lib_rate, 1),
               fused_mfma_TFLOPs=round(2 * flop / us["fused"] / 1e6, 1),
               fused_ref_mfma_TFLOPs=round(3 * flop / us["fused_ref"] / 1e6, 1),
               fused_frac_of_2x_matmul=round(2 * us["bf16_matmul"] / us["fused"], 3),
               fused_ref_frac_of_3x_matmul=round(3 * us["bf16_matmul"] / us["fused_ref"], 3),
               sums_fused_vs_composed=agree)
    return out


def search_block(T, L, n_grid, rounds):
    """One Llama-3-8B decoder block's four layer groups (q/k/v 4096+1024+1024 x 4096, o 4096 x 4096,
    gate/up 2 x 14336 x 4096, down 4096 x 14336): quantize_layer_group with the diagonal loss and
    with loss="output", host-timed around a device synchronize (the call has host work of its own)."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    q = AWQQuantizer(bits=4, group_size=L, symmetric=False, device="cuda:0", scale_method="awq", search_grid=n_grid,
                     logger_level="ERROR")
    groups = {"attn_in": ([4096, 1024, 1024], 4096), "attn_out": ([4096], 4096), "mlp_in": ([14336, 14336], 4096),
              "mlp_out": ([4096], 14336)}
    out = {"tokens": T, "group_size": L, "candidates": n_grid}
    for loss in ("diag", "output"):
        total = 0.0
        for name, (rows, K) in groups.items():
            ws = {f"w{i}": (torch.randn(r, K, device=dev, generator=g) * 0.02).bfloat16() for i, r in enumerate(rows)}
            x = (torch.randn(T, K, device=dev, generator=g) * (0.25 + 4 * torch.rand(K, device=dev, generator=g) ** 3)).bfloat16()
            ts = []
            for _ in range(rounds + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                q.quantize_layer_group(ws, x, loss=loss)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[f"{loss}_{name}_ms"] = round(statistics.median(ts[1:]), 2)
            total += statistics.median(ts[1:])
            del ws
            torch.cuda.empty_cache()
        out[f"{loss}_block_ms"] = round(total, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="14336x4096,4096x14336,128256x4096")
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--group-size", type=int, default=128)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0, help="least length of a timed window")
    ap.add_argument("--footprint-mib", type=int, default=1024,
                    help="weights cycled through before a tensor is read again (0: one copy, cache-warm)")
    ap.add_argument("--search-block", action="store_true", help="also time one decoder block's scale searches")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("output_error_bench: needs a GPU (no CPU fallback; a CPU timing would say nothing)")
    _hip.require_device(torch.device("cuda", 0))
    for s in [v for v in a.shapes.split(",") if v]:
        N, K = (int(v) for v in s.lower().split("x"))
        print(json.dumps(bench_shape(N, K, a.tokens, a.group_size, a.bits, a.rounds, a.window_ms,
                                     a.footprint_mib << 20)), flush=True)
        torch.cuda.empty_cache()
    if a.search_block:
        print(json.dumps({"search_block": search_block(a.tokens, a.group_size, 20, 3)}), flush=True)


if __name__ == "__main__":
    main()
