#!/usr/bin/env python3
"""Throughput of the AutoAWQ "GEMM"-layout import (include/awq_hip.h awq_import_autoawq_gemm,
csrc/awq_import.hip) against its yardstick, the export of the same tensor (awq_export_autoawq_gemm:
the same bytes with the mirrored access pattern), measured in one process.

Per shape: `copies` sets of packed + GEMM-layout buffers (enough that a set is touched again only
after more than `--footprint` bytes of other traffic, so no launch finds its input in the 256 MB
Infinity Cache); both calls are warmed on every set; then `--rounds` rounds, each one timed window
of imports followed by one of exports, every window at least `--window-ms` long (device events
around back-to-back launches cycling over the sets, no allocation inside).  Reported: the median
window of each call in us per launch, the spread (min .. max over the rounds), bytes moved (every
input word read once + every output word written once) over the median against 8 TB/s, and the
ratio import / export.  Before timing, import(export(p)) is compared with p word for word.

  python scripts/import_bench.py [--rounds 7] [--window-ms 50] [--log profiles/import_bench.log]
                                 [--lib awq-converter_amd/awq_quantizer/_lib/ab/libawq_hip_X.so]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "awq-converter_amd")]
import torch  # noqa: E402

SHAPES = {"lm_head": (128256, 4096), "gate/up_proj": (14336, 4096)}
GS = 128


def window(fn, sets, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(sets[i % len(sets)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--footprint", type=int, default=1 << 30, help="bytes of other traffic between two uses of a set")
    ap.add_argument("--lib", default=None, help="A/B build of the library (scripts/build_variant.sh)")
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from awq_quantizer import _hip
    if args.lib:
        _hip.load_library(os.path.join(ROOT, args.lib))
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    lines = []
    for name, (N, K) in SHAPES.items():
        G = K // GS
        g = torch.Generator(device=dev).manual_seed(N + K)
        info = torch.iinfo(torch.int32)
        shapes = {"qweight": ((N, K // 8), torch.int32), "qzeros": ((N, (G + 7) // 8), torch.int32),
                  "scales": ((N, G), torch.float16)}
        shapes_t = {"qweight": ((K, N // 8), torch.int32), "qzeros": ((G, N // 8), torch.int32),
                    "scales": ((G, N), torch.float16)}
        nbytes = sum(torch.Size(s).numel() * torch.empty((), dtype=d).element_size()
                     for s, d in list(shapes.values()) + list(shapes_t.values()))
        copies = max(2, -(-args.footprint // nbytes) + 1)
        sets = []
        for _ in range(copies):
            p = {"qweight": torch.randint(info.min, info.max, shapes["qweight"][0], generator=g, device=dev,
                                          dtype=torch.int32),
                 "qzeros": torch.randint(info.min, info.max, shapes["qzeros"][0], generator=g, device=dev,
                                         dtype=torch.int32),
                 "scales": torch.randn(shapes["scales"][0], generator=g, device=dev).half()}
            t = {k: torch.empty(s, dtype=d, device=dev) for k, (s, d) in shapes_t.items()}
            back = {k: torch.empty(s, dtype=d, device=dev) for k, (s, d) in shapes.items()}
            sets.append((p, t, back))

        def export(s):
            p, t, _ = s
            _hip.export_autoawq_gemm(p["qweight"], p["qzeros"], p["scales"], N, K, GS, 4, t["qweight"], t["qzeros"],
                                     t["scales"])

        def imp(s):
            _, t, back = s
            _hip.import_autoawq_gemm(t["qweight"], t["qzeros"], t["scales"], N, K, GS, 4, back["qweight"],
                                     back["qzeros"], back["scales"])

        for s in sets:                               # warm-up of both calls on every set, and the round trip
            export(s)
            imp(s)
        torch.cuda.synchronize()
        p, _, back = sets[0]
        if not (torch.equal(back["qweight"], p["qweight"]) and torch.equal(back["qzeros"], p["qzeros"])
                and torch.equal(back["scales"].view(torch.int16), p["scales"].view(torch.int16))):
            raise SystemExit(f"{name}: import(export(p)) != p")
        n = {}
        for key, fn in (("import", imp), ("export", export)):    # launches per window from a short probe
            us = window(fn, sets, 4 * copies)
            n[key] = max(copies, int(args.window_ms * 1e3 / us * 1.1) + 1)
        us = {"import": [], "export": []}
        for _ in range(args.rounds):
            for key, fn in (("import", imp), ("export", export)):
                us[key].append(window(fn, sets, n[key]))
        out = {"lib": args.lib or "product", "tensor": name, "N": N, "K": K, "group_size": GS, "bytes": nbytes, "copies": copies,
               "rounds": args.rounds}
        for key in ("import", "export"):
            med = statistics.median(us[key])
            out[key] = {"launches_per_window": n[key], "window_ms": round(med * n[key] / 1e3, 1),
                        "median_us": round(med, 2), "min_us": round(min(us[key]), 2), "max_us": round(max(us[key]), 2),
                        "GBs": round(nbytes / med / 1e3, 1), "frac_8TBs": round(nbytes / med / 1e3 / 8000, 3)}
        out["import_over_export"] = round(out["import"]["median_us"] / out["export"]["median_us"], 4)
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
        del sets
        torch.cuda.empty_cache()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
