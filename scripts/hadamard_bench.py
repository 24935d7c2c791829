#!/usr/bin/env python3
"""awq_hadamard_rows / awq_hadamard_cols against awq_stream_copy of the same bytes
and against the dense product W @ Q in torch, interleaved in one process on the same tensors (HIP
events, `--rounds` rounds of windows of at least `--window-ms` each, medians; every case cycles over
enough copies of the tensor that no launch finds its input in the Infinity Cache).  One JSON line per
shape: GB/s of each transform (bytes read + written of the matrix alone), its rate over the copy's,
and the dense product's time over the transform's.

  python scripts/hadamard_bench.py [--shapes 4096x4096,14336x4096,4096x14336] [--dtype bf16]
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
from awq_quantizer.rotation import _device_mix, hadamard_factor  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def bench_shape(R, K, dtype, rounds, window_ms, footprint):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(R + K)
    nbytes = R * K * torch.empty((), dtype=dtype).element_size()
    reps = max(1, -(-footprint // nbytes))
    ws = [(torch.randn(R, K, device=dev, generator=g) * 0.02).to(dtype) for _ in range(reps)]
    out, stream, turn = torch.empty_like(ws[0]), _hip.stream_ptr(dev), {"i": 0}
    cases = {}

    def pick():
        turn["i"] = (turn["i"] + 1) % reps
        return ws[turn["i"]]

    def axis_cases(axis, n):
        m, _, M = hadamard_factor(n)
        mix = _device_mix(m, dev)
        pre = (torch.randint(0, 2, (n,), device=dev, generator=g) * 2 - 1).float()
        H = torch.ones(1, 1, dtype=torch.float64)
        while H.shape[0] < n // m:
            H = torch.cat((torch.cat((H, H), 1), torch.cat((H, -H), 1)), 0)
        Q = (pre.cpu().double()[:, None] * torch.kron(M if M is not None else torch.ones(1, 1, dtype=torch.float64), H)
             / n ** 0.5).to(dev).float()
        if axis == "rows":
            cases["rows"] = lambda: _hip.hadamard_rows(pick(), n, m, pre, mix, out)
            cases["rows_dense"] = lambda: torch.matmul(pick().float(), Q).to(dtype)
        else:
            cases["cols"] = lambda: _hip.hadamard_cols(pick(), n, m, pre, mix, out)
            cases["cols_dense"] = lambda: torch.matmul(Q.t(), pick().float()).to(dtype)

    axis_cases("rows", K)
    axis_cases("cols", R)
    cases["copy"] = lambda: _hip.stream_copy(pick(), out, stream)
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
    r = {"device": torch.cuda.get_device_name(0), "rows": R, "K": K, "dtype": str(dtype).split(".")[-1],
         "bytes_read_plus_written": 2 * nbytes, "tensor_copies_cycled": reps,
         "cols_work_bytes": int(_hip.load_library().awq_hadamard_cols_work_bytes(_hip.AWQ_DTYPE[dtype], R, K, R,
                                                                                 hadamard_factor(R)[0]))}
    for k in cases:
        r[k + "_us"] = round(us[k], 1)
        r[k + "_us_min_max"] = [round(min(times[k]), 1), round(max(times[k]), 1)]
    for k in ("rows", "cols", "copy"):
        r[k + "_GBps"] = round(2 * nbytes / us[k] * 1e-3, 1)
    for k in ("rows", "cols"):
        r[k + "_over_copy_rate"] = round(us["copy"] / us[k], 3)
        r[k + "_speedup_over_dense"] = round(us[k + "_dense"] / us[k], 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x4096,14336x4096,4096x14336")
    ap.add_argument("--dtype", default="bf16", choices=sorted(DTYPES))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0, help="least length of a timed window")
    ap.add_argument("--footprint-mib", type=int, default=1024,
                    help="weights cycled through before a tensor is read again (0: one copy, cache-warm)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hadamard_bench: needs a GPU (no CPU fallback; a CPU timing would say nothing)")
    _hip.require_device(torch.device("cuda", 0))
    for sh in a.shapes.split(","):
        R, K = (int(v) for v in sh.lower().split("x"))
        print(json.dumps(bench_shape(R, K, DTYPES[a.dtype], a.rounds, a.window_ms, a.footprint_mib << 20)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
