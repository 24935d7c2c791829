#!/usr/bin/env python3
"""awq_quantize_mxfp4 / awq_dequantize_mxfp4 / awq_mxfp4_error against awq_stream_copy of
the weight's bytes and against the int4 streaming kernel (quantize_packed's launch, group size 128) on
the same tensors, every case into preallocated buffers, interleaved in one process (HIP events,
`--rounds` rounds of windows of at least `--window-ms` each, medians; every case cycles over enough copies of the tensor that no launch finds its input in the Infinity Cache).  One JSON
line per shape: GB/s of each entry over the bytes its definition reads plus writes (the error entry's
workspace traffic is not counted), and that rate over the copy's.

  python scripts/mxfp4_bench.py [--shapes 4096x4096,14336x4096,4096x14336] [--dtype bf16] [--rule floor]
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
from awq_quantizer.quantization.awq import AWQQuantizer  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def bench_shape(R, K, dtype, rule, rounds, window_ms, footprint):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(R + K)
    n, esz = R * K, torch.empty((), dtype=dtype).element_size()
    reps = max(1, -(-footprint // (n * esz)))
    ws = [(torch.randn(R, K, device=dev, generator=g) * 0.02).to(dtype) for _ in range(reps)]
    q = AWQQuantizer(bits=4, group_size=128, symmetric=False, device="cuda", logger_level="ERROR")
    codes = torch.empty((R, K // 2), dtype=torch.uint8, device=dev)
    scales = torch.empty((R, K // 32), dtype=torch.uint8, device=dev)
    out, stream, turn = torch.empty_like(ws[0]), _hip.stream_ptr(dev), {"i": 0}
    _hip.quantize_mxfp4(ws[0], rule, codes, scales)
    # every case launches into preallocated buffers: the entries themselves, not their allocating wrappers
    lib = _hip.load_library()
    err_out = torch.empty(lib.awq_mxfp4_error_out_bytes(R, K) // 8 + 1, dtype=torch.float64, device=dev)
    int4 = q._packed_outputs(ws[0])
    if not _hip.packs_directly(dtype, R, K, q.group_size):
        raise SystemExit(f"mxfp4_bench: {R}x{K} {dtype} does not take the int4 streaming kernel")

    def error(w):
        _hip.check(lib.awq_mxfp4_error(_hip.ptr(w), _hip.AWQ_DTYPE[dtype], _hip.ptr(codes), _hip.ptr(scales), R, K,
                                       _hip.ptr(err_out), stream), "awq_mxfp4_error")

    def pick():
        turn["i"] = (turn["i"] + 1) % reps
        return ws[turn["i"]]

    packed = n // 2 + n // 32
    cases = {"quantize": (lambda: _hip.quantize_mxfp4(pick(), rule, codes, scales), n * esz + packed),
             "dequantize": (lambda: _hip.dequantize_mxfp4(codes, scales, out), packed + n * esz),
             "error": (lambda: error(pick()), n * esz + packed),
             "int4_packed": (lambda: q._launch(pick(), R, K, q.group_size, qweight=int4["qweight"], qzeros=int4["qzeros"],
                                               scales=int4["scales"]), n * esz + n // 2 + n // 128 * 2 + n // 256),
             "copy": (lambda: _hip.stream_copy(pick(), out, stream), 2 * n * esz)}
    iters = {}
    for name, (fn, _) in cases.items():     # warm-up of every case on this shape, and its window length
        fn()
        torch.cuda.synchronize()
        iters[name] = max(3, int(window_ms * 1e3 / max(timed(fn, 3), 1.0)) + 1)
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for name, (fn, _) in cases.items():
            times[name].append(timed(fn, iters[name]))
    us = {k: statistics.median(v) for k, v in times.items()}
    rate = {k: cases[k][1] / us[k] * 1e-3 for k in cases}
    r = {"device": torch.cuda.get_device_name(0), "rows": R, "K": K, "dtype": str(dtype).split(".")[-1],
         "scale_rule": rule, "tensor_copies_cycled": reps}
    for k in cases:
        r[k + "_us"] = round(us[k], 1)
        r[k + "_us_min_max"] = [round(min(times[k]), 1), round(max(times[k]), 1)]
        r[k + "_GBps"] = round(rate[k], 1)
        if k != "copy":
            r[k + "_over_copy_rate"] = round(rate[k] / rate["copy"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x4096,14336x4096,4096x14336")
    ap.add_argument("--dtype", default="bf16", choices=sorted(DTYPES))
    ap.add_argument("--rule", default="floor", choices=sorted(_hip.MXFP4_RULES))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0, help="least length of a timed window")
    ap.add_argument("--footprint-mib", type=int, default=1024,
                    help="weights cycled through before a tensor is read again (0: one copy, cache-warm)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_bench: needs a GPU (no CPU fallback; a CPU timing would say nothing)")
    _hip.require_device(torch.device("cuda", 0))
    for sh in a.shapes.split(","):
        R, K = (int(v) for v in sh.lower().split("x"))
        print(json.dumps(bench_shape(R, K, DTYPES[a.dtype], a.rule, a.rounds, a.window_ms, a.footprint_mib << 20)),
              flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
