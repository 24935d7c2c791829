#!/usr/bin/env python3
"""awq_fold_rows (the scale fold, out = RN_D(RN_f32(w / row_scale[r]))) against awq_stream_copy of
the same bytes — the 1 : 1 read : write streaming structure the fold kernel shares — interleaved
in one process on the same tensors (HIP events, `--rounds` rounds of windows of at least
`--window-ms` each, medians; both cases cycle over enough copies of the tensor that no launch
finds its input in the Infinity Cache, and write the same output buffer).
Default shape: Llama-3-8B's up projection, 14336 x 4096 bf16.  One JSON line per shape with
`fold_over_copy_rate` = copy time / fold time (1.0: the fold streams as fast as the plain copy).

  python scripts/fold_bench.py [--shapes 14336x4096] [--dtype bf16]
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

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def bench_shape(rows, K, dtype, rounds, window_ms, footprint):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(rows + K)
    nbytes = rows * K * torch.empty((), dtype=dtype).element_size()
    reps = max(1, -(-footprint // nbytes))
    ws = [(torch.randn(rows, K, device=dev, generator=g) * 0.02).to(dtype) for _ in range(reps)]
    s = torch.exp(torch.randn(rows, device=dev, generator=g)).float()
    out = torch.empty_like(ws[0])
    stream = _hip.stream_ptr(dev)
    turn = {"i": 0}

    def pick():
        turn["i"] = (turn["i"] + 1) % reps
        return ws[turn["i"]]

    def fold():
        _hip.fold_rows(pick(), s, out=out)

    def copy():
        _hip.stream_copy(pick(), out, stream)

    cases = {"fold": fold, "copy": copy}
    iters = {}
    for name, fn in cases.items():          # warm-up of every case on this shape, and its window length
        fn()
        torch.cuda.synchronize()
        iters[name] = max(3, int(window_ms * 1e3 / max(timed(fn, 3), 1.0)) + 1)
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for name, fn in cases.items():
            times[name].append(timed(fn, iters[name]))
    us = {k: statistics.median(v) for k, v in times.items()}
    # the timed output is the definition's (torch CPU), on the copy folded last
    turn["i"] = reps - 1
    fold()
    want = (ws[0][:64].cpu().float() / s[:64].cpu()[:, None]).to(dtype)
    it = torch.int32 if dtype == torch.float32 else torch.int16
    exact = bool(torch.equal(out[:64].cpu().view(it), want.view(it)))
    r = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
         "rows": rows, "K": K, "dtype": str(dtype).split(".")[-1],
         "bytes_read_plus_written": 2 * nbytes, "tensor_copies_cycled": reps, "launches_per_window": iters,
         "bit_exact_first_64_rows": exact}
    for k in cases:
        r[k + "_us"] = round(us[k], 1)
        r[k + "_us_min_max"] = [round(min(times[k]), 1), round(max(times[k]), 1)]
        r[k + "_TBps"] = round(2 * nbytes / us[k] * 1e-6, 3)
    r["fold_over_copy_rate"] = round(us["copy"] / us["fold"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="14336x4096")
    ap.add_argument("--dtype", default="bf16", choices=sorted(DTYPES))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0, help="least length of a timed window")
    ap.add_argument("--footprint-mib", type=int, default=1024,
                    help="weights cycled through before a tensor is read again (0: one copy, cache-warm)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fold_bench: needs a GPU (no CPU fallback; a CPU timing would say nothing)")
    _hip.require_device(torch.device("cuda", 0))
    for sh in a.shapes.split(","):
        rows, K = (int(v) for v in sh.lower().split("x"))
        print(json.dumps(bench_shape(rows, K, DTYPES[a.dtype], a.rounds, a.window_ms, a.footprint_mib << 20)),
              flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
