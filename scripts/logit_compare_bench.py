#!/usr/bin/env python3
"""awq_logit_compare (the evaluation tail's fused comparison of two logit matrices) against the two
things it is quoted against, interleaved in one process on the same data (HIP events, `--rounds`
rounds of windows of at least `--window-ms` each, medians and min / max; every case cycles over
enough copies of the inputs, at least `--footprint-mib` in all, that no launch finds them in the
Infinity Cache):
  * torch: the composition a user would write — .float() of both, two log_softmax, gather of the
    targets, the KL sum exp(lr) * (lr - lq), two argmax;
  * copy: awq_stream_copy over the same 2 * T * V * 2 bytes (it also writes them; the fused call
    writes 20 bytes per row), the tree's measure of what the memory system gives a streaming kernel.
Default: bf16 at (T, V) = (2048, 32000), (2048, 128256), (2048, 151936).  One JSON line per shape.

  python scripts/logit_compare_bench.py [--shapes 2048x32000,2048x128256,2048x151936]
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


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def bench_shape(T, V, rounds, window_ms, footprint):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(V)
    pair_bytes = 2 * T * V * 2
    reps = max(2, -(-footprint // pair_bytes))
    refs, qs = [], []
    for _ in range(reps):
        r = torch.randn(T, V, device=dev, generator=g) * 4
        refs.append(r.bfloat16())
        qs.append((r + torch.randn(T, V, device=dev, generator=g) * 0.3).bfloat16())
        del r
    targets = torch.randint(0, V, (T,), device=dev, generator=g)
    f32 = {k: torch.empty(T, dtype=torch.float32, device=dev) for k in ("nll_ref", "nll_q", "kl")}
    i32 = {k: torch.empty(T, dtype=torch.int32, device=dev) for k in ("argmax_ref", "argmax_q")}
    dst = torch.empty(2 * T * V, dtype=torch.bfloat16, device=dev)
    stream = _hip.stream_ptr(dev)
    turn = {"i": 0}
    keep = {}

    def pick():
        turn["i"] = (turn["i"] + 1) % reps
        return refs[turn["i"]], qs[turn["i"]]

    def fused():
        r, q = pick()
        _hip.logit_compare(r, q, targets, **f32, **i32)

    def composed():
        r, q = pick()
        lr, lq = torch.log_softmax(r.float(), -1), torch.log_softmax(q.float(), -1)
        keep["nll_ref"] = -lr.gather(1, targets[:, None])[:, 0]
        keep["nll_q"] = -lq.gather(1, targets[:, None])[:, 0]
        keep["kl"] = (lr.exp() * (lr - lq)).sum(-1)
        keep["argmax_ref"], keep["argmax_q"] = r.argmax(-1), q.argmax(-1)

    def copy():                                  # the same bytes read: both matrices of the pair
        r, q = pick()
        _hip.stream_copy(r.reshape(-1), dst[: T * V], stream)
        _hip.stream_copy(q.reshape(-1), dst[T * V:], stream)

    cases = {"fused": fused, "torch": composed, "copy": copy}
    iters = {}
    for name, fn in cases.items():
        fn()
        torch.cuda.synchronize()
        iters[name] = max(3, int(window_ms * 1e3 / max(timed(fn, 3), 1.0)) + 1)
    turn["i"] = reps - 1                         # both on copy 0: the two paths' results side by side
    fused()
    turn["i"] = reps - 1
    composed()
    torch.cuda.synchronize()
    agree = {k: float((f32[k].double() - keep[k].double()).abs().max()) for k in f32}
    agree["argmax_equal"] = bool(torch.equal(i32["argmax_ref"].long(), keep["argmax_ref"])
                                 and torch.equal(i32["argmax_q"].long(), keep["argmax_q"]))
    keep.clear()
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for name, fn in cases.items():
            times[name].append(timed(fn, iters[name]))
    us = {k: statistics.median(v) for k, v in times.items()}
    out = {"T": T, "V": V, "dtype": "bf16", "pairs_cycled": reps, "bytes_read": pair_bytes, "launches_per_window": iters}
    for k in cases:
        out[k + "_us"] = round(us[k], 1)
        out[k + "_us_min_max"] = [round(min(times[k]), 1), round(max(times[k]), 1)]
    out.update(fused_read_TBps=round(pair_bytes / us["fused"] / 1e6, 3),
               copy_read_TBps=round(pair_bytes / us["copy"] / 1e6, 3),
               copy_over_fused=round(us["copy"] / us["fused"], 3),
               speedup_over_torch=round(us["torch"] / us["fused"], 2),
               max_abs_difference_fused_vs_torch=agree)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048x32000,2048x128256,2048x151936")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0, help="least length of a timed window")
    ap.add_argument("--footprint-mib", type=int, default=1024, help="least bytes of inputs cycled through")
    args = ap.parse_args()
    _hip.require_device(torch.device("cuda", 0))
    for shape in args.shapes.split(","):
        T, V = (int(v) for v in shape.split("x"))
        print(json.dumps(bench_shape(T, V, args.rounds, args.window_ms, args.footprint_mib << 20)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
