#!/usr/bin/env python3
"""Throughput of the GPTQ-layout export and import (include/awq_hip.h awq_export_gptq /
awq_import_gptq, csrc/awq_gptq.hip) beside their yardstick, the AutoAWQ pair
(awq_export_autoawq_gemm / awq_import_autoawq_gemm), on the same packed buffers in one process:
both pairs move the same bytes (the GPTQ export also writes g_idx, 4 K bytes).

Per shape: `copies` sets of packed + GPTQ-layout + GEMM-layout buffers (enough that a set is touched
again only after more than `--footprint` bytes of other traffic, so no launch finds its input in the
256 MB Infinity Cache); all four calls are warmed on every set; then `--rounds` rounds, each one
timed window per call in turn (interleaved, so drift hits all four alike), every window at least
`--window-ms` long (device events around back-to-back launches cycling over the sets, no allocation
inside).  Reported per call: the median window in us per launch, the spread over the rounds, bytes
moved (every input word read once + every output word written once) over the median against
8 TB/s; and the ratios gptq / autoawq.  Before timing, both round trips are compared with the
packed input word for word.

  python scripts/gptq_export_bench.py [--rounds 7] [--window-ms 50] [--log profiles/gptq_export_bench.log]
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
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from awq_quantizer import _hip
    from awq_quantizer.layout import gptq_shapes, row_shapes
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    lines = []
    for name, (N, K) in SHAPES.items():
        G = K // GS
        g = torch.Generator(device=dev).manual_seed(N + K)
        info = torch.iinfo(torch.int32)
        rs, gs = row_shapes(N, K, GS, 4), gptq_shapes(N, K, GS)
        i32, f16 = torch.int32, torch.float16
        shapes = {"qweight": (rs["qweight"], i32), "qzeros": (rs["qzeros"], i32), "scales": (rs["scales"], f16)}
        shapes_g = {"qweight": (gs["qweight"], i32), "qzeros": (gs["qzeros"], i32), "scales": (gs["scales"], f16)}
        shapes_a = {"qweight": ((K, N // 8), i32), "qzeros": ((G, N // 8), i32), "scales": ((G, N), f16)}
        size = lambda d: sum(torch.Size(s).numel() * torch.empty((), dtype=t).element_size() for s, t in d.values())
        nbytes = size(shapes) + size(shapes_g)          # per call (= the AutoAWQ pair's: the same word counts)
        assert size(shapes_g) == size(shapes_a)
        copies = max(2, -(-args.footprint // nbytes) + 1)
        sets = []
        for _ in range(copies):
            p = {"qweight": torch.randint(info.min, info.max, shapes["qweight"][0], generator=g, device=dev, dtype=i32),
                 "qzeros": torch.randint(info.min, info.max, shapes["qzeros"][0], generator=g, device=dev, dtype=i32),
                 "scales": torch.randn(shapes["scales"][0], generator=g, device=dev).half()}
            tg = {k: torch.empty(s, dtype=d, device=dev) for k, (s, d) in shapes_g.items()}
            tg["g_idx"] = torch.empty(K, dtype=i32, device=dev)
            ta = {k: torch.empty(s, dtype=d, device=dev) for k, (s, d) in shapes_a.items()}
            back = {k: torch.empty(s, dtype=d, device=dev) for k, (s, d) in shapes.items()}
            sets.append((p, tg, ta, back))

        def gptq_export(s):
            p, t = s[0], s[1]
            _hip.export_gptq(p["qweight"], p["qzeros"], p["scales"], N, K, GS, 4, False, 1, t["qweight"], t["qzeros"],
                             t["scales"], t["g_idx"])

        def gptq_import(s):
            t, back = s[1], s[3]
            _hip.import_gptq(t["qweight"], t["qzeros"], t["scales"], N, K, GS, 4, False, 1, back["qweight"],
                             back["qzeros"], back["scales"])

        def awq_export(s):
            p, t = s[0], s[2]
            _hip.export_autoawq_gemm(p["qweight"], p["qzeros"], p["scales"], N, K, GS, 4, t["qweight"], t["qzeros"],
                                     t["scales"])

        def awq_import(s):
            t, back = s[2], s[3]
            _hip.import_autoawq_gemm(t["qweight"], t["qzeros"], t["scales"], N, K, GS, 4, back["qweight"],
                                     back["qzeros"], back["scales"])

        def round_trip_ok(s):
            p, back = s[0], s[3]
            return (torch.equal(back["qweight"], p["qweight"]) and torch.equal(back["qzeros"], p["qzeros"])
                    and torch.equal(back["scales"].view(torch.int16), p["scales"].view(torch.int16)))

        for pair in ((gptq_export, gptq_import), (awq_export, awq_import)):   # warm-up on every set; the round trips
            for s in sets:
                pair[0](s)
                pair[1](s)
            torch.cuda.synchronize()
            if not round_trip_ok(sets[0]):
                raise SystemExit(f"{name}: {pair[1].__name__}({pair[0].__name__}(p)) != p")
            for s in sets:
                for t in s[3].values():
                    t.zero_()
        calls = (("gptq_export", gptq_export), ("autoawq_export", awq_export), ("gptq_import", gptq_import),
                 ("autoawq_import", awq_import))
        n = {}
        for key, fn in calls:                            # launches per window from a short probe
            us = window(fn, sets, 4 * copies)
            n[key] = max(copies, int(args.window_ms * 1e3 / us * 1.1) + 1)
        us = {key: [] for key, _ in calls}
        for _ in range(args.rounds):
            for key, fn in calls:
                us[key].append(window(fn, sets, n[key]))
        out = {"tensor": name, "N": N, "K": K, "group_size": GS, "bytes": nbytes, "copies": copies, "rounds": args.rounds}
        for key, _ in calls:
            med = statistics.median(us[key])
            out[key] = {"launches_per_window": n[key], "window_ms": round(med * n[key] / 1e3, 1),
                        "median_us": round(med, 2), "min_us": round(min(us[key]), 2), "max_us": round(max(us[key]), 2),
                        "GBs": round(nbytes / med / 1e3, 1), "frac_8TBs": round(nbytes / med / 1e3 / 8000, 3)}
        out["gptq_over_autoawq_export"] = round(out["gptq_export"]["median_us"] / out["autoawq_export"]["median_us"], 4)
        out["gptq_over_autoawq_import"] = round(out["gptq_import"]["median_us"] / out["autoawq_import"]["median_us"], 4)
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
