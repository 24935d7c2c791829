#!/usr/bin/env python3
"""Throughput of the GPTQ act-order data path (include/awq_hip.h awq_gptq_permute_rows /
awq_dequantize_gptq, csrc/awq_gptq_actorder.hip) beside its yardsticks, on the
same buffers in one process:
  export / import with desc_act = true (awq_export_gptq into a temporary + the gather; the gather +
      awq_import_gptq) against the desc_act = false pair, and the gather alone;
  awq_dequantize_gptq to fp16 with a random balanced g_idx against today's three steps
      (awq_import_gptq, awq_dequantize_packed, a cast and index_select), and with the trivial g_idx
      against awq_dequantize_packed alone (fp32 out, the 1 : 8 stream).

As scripts/gptq_export_bench.py: `copies` sets of buffers cycled so that no launch finds its input
in the 256 MB Infinity Cache, every call warmed on every set, `--rounds` interleaved rounds of
device-event windows of at least `--window-ms`; median, min and max in us per call.  Before timing
the act-order round trip is compared with the packed input word for word and the fused dequantize
with the three-step route bit for bit.  `--only gather` times the gather alone (a counter pass
wraps exactly that: FETCH_SIZE / WRITE_SIZE against the 2 x K/8 x N x 4 algorithmic bytes).

  python scripts/gptq_actorder_bench.py [--rounds 7] [--window-ms 50] [--only gather] [--log FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "awq-converter_amd")]
import torch  # noqa: E402

from gptq_export_bench import GS, SHAPES, window  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--footprint", type=int, default=1 << 30, help="bytes of other traffic between two uses of a set")
    ap.add_argument("--only", default=None, choices=["gather"])
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from awq_quantizer import _hip
    from awq_quantizer.layout import gptq_shapes, row_shapes
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    i32, f16 = torch.int32, torch.float16
    info = torch.iinfo(i32)
    lines = []
    for name, (N, K) in SHAPES.items():
        g = torch.Generator(device=dev).manual_seed(N + K)
        rs, gs = row_shapes(N, K, GS, 4), gptq_shapes(N, K, GS)
        perm = torch.randperm(K, generator=g, device=dev).to(i32)
        g_idx, inv = torch.empty_like(perm), torch.empty_like(perm)
        _hip.gptq_gidx_from_perm(perm, GS, g_idx, inv)
        trivial = (torch.arange(K, device=dev) // GS).to(i32)
        words = N * K // 8 * 4
        per_set = 3 * words + N * K * 4 + 2 * N * K * 2      # packed + two GPTQ qweights + fp32 and two fp16 weights
        copies = max(2, -(-args.footprint // per_set) + 1)
        sets = []
        for _ in range(copies):
            rnd = lambda sh: torch.randint(info.min, info.max, sh, generator=g, device=dev, dtype=i32)
            p = {"qweight": rnd(rs["qweight"]), "qzeros": rnd(rs["qzeros"]),
                 "scales": torch.rand(rs["scales"], generator=g, device=dev).half()}
            t = {k: torch.empty(gs[k], dtype=f16 if k == "scales" else i32, device=dev) for k in ("qweight", "qzeros", "scales")}
            sets.append({"p": p, "t": t, "tmp": torch.empty_like(t["qweight"]), "gi": torch.empty(K, dtype=i32, device=dev),
                         "back": {k: torch.empty_like(v) for k, v in p.items()},
                         "w32": torch.empty((N, K), device=dev), "w16": torch.empty((N, K), dtype=f16, device=dev),
                         "w16b": torch.empty((N, K), dtype=f16, device=dev)})

        def export_false(s):
            p, t = s["p"], s["t"]
            _hip.export_gptq(p["qweight"], p["qzeros"], p["scales"], N, K, GS, 4, False, 1, t["qweight"], t["qzeros"],
                             t["scales"], s["gi"])

        def export_true(s):
            p, t = s["p"], s["t"]
            _hip.export_gptq(p["qweight"], p["qzeros"], p["scales"], N, K, GS, 4, False, 1, s["tmp"], t["qzeros"],
                             t["scales"], None)
            _hip.gptq_gidx_from_perm(perm, GS, s["gi"], inv)
            _hip.gptq_permute_rows(s["tmp"], inv, t["qweight"])

        def import_false(s):
            t, b = s["t"], s["back"]
            _hip.import_gptq(t["qweight"], t["qzeros"], t["scales"], N, K, GS, 4, False, 1, b["qweight"], b["qzeros"],
                             b["scales"])

        def import_true(s):
            t, b = s["t"], s["back"]
            _hip.gptq_permute_rows(t["qweight"], perm, s["tmp"])
            _hip.import_gptq(s["tmp"], t["qzeros"], t["scales"], N, K, GS, 4, False, 1, b["qweight"], b["qzeros"],
                             b["scales"])

        def gather(s):
            _hip.gptq_permute_rows(s["t"]["qweight"], perm, s["tmp"])

        def fused(s):
            t = s["t"]
            _hip.dequantize_gptq(t["qweight"], t["qzeros"], t["scales"], g_idx, 1, s["w16"])

        def three_steps(s):
            import_true(s)
            b = s["back"]
            _hip.dequantize_packed(b["qweight"], b["qzeros"], b["scales"], N, K, GS, 4, False, s["w32"])
            torch.index_select(s["w32"].half(), 1, inv.long(), out=s["w16b"])

        def fused_trivial(s):
            t = s["t"]
            _hip.dequantize_gptq(t["qweight"], t["qzeros"], t["scales"], trivial, 1, s["w32"])

        def packed_alone(s):
            b = s["back"]
            _hip.dequantize_packed(b["qweight"], b["qzeros"], b["scales"], N, K, GS, 4, False, s["w32"])

        s0 = sets[0]
        export_true(s0)
        import_true(s0)
        fused(s0)
        three_steps(s0)
        torch.cuda.synchronize()
        if not (torch.equal(s0["back"]["qweight"], s0["p"]["qweight"]) and torch.equal(s0["back"]["qzeros"], s0["p"]["qzeros"])):
            raise SystemExit(f"{name}: import(export(p)) with desc_act true != p")
        same = (s0["w16"].view(torch.int16) == s0["w16b"].view(torch.int16)) | (s0["w16"].isnan() & s0["w16b"].isnan())
        if not bool(same.all()):
            raise SystemExit(f"{name}: awq_dequantize_gptq differs from the three-step route")
        calls = [("gather", gather)] if args.only else [
            ("export_desc_act", export_true), ("export", export_false), ("import_desc_act", import_true),
            ("import", import_false), ("gather", gather), ("dequantize_gptq_fp16", fused), ("three_steps_fp16", three_steps),
            ("dequantize_gptq_trivial_fp32", fused_trivial), ("dequantize_packed_fp32", packed_alone)]
        for _, fn in calls:
            for s in sets:
                fn(s)
        torch.cuda.synchronize()
        n = {}
        for key, fn in calls:                            # launches per window from a short probe
            n[key] = max(copies, int(args.window_ms * 1e3 / window(fn, sets, 2 * copies) * 1.1) + 1)
        us = {key: [] for key, _ in calls}
        for _ in range(args.rounds):
            for key, fn in calls:
                us[key].append(window(fn, sets, n[key]))
        out = {"tensor": name, "N": N, "K": K, "group_size": GS, "copies": copies, "rounds": args.rounds,
               "gather_bytes": 2 * words}
        for key, _ in calls:
            med = statistics.median(us[key])
            out[key] = {"calls_per_window": n[key], "window_ms": round(med * n[key] / 1e3, 1), "median_us": round(med, 2),
                        "min_us": round(min(us[key]), 2), "max_us": round(max(us[key]), 2)}
        out["gather"]["GBs"] = round(2 * words / out["gather"]["median_us"] / 1e3, 1)
        if not args.only:
            ratio = lambda a, b: round(out[a]["median_us"] / out[b]["median_us"], 4)
            out.update(export_ratio=ratio("export_desc_act", "export"), import_ratio=ratio("import_desc_act", "import"),
                       fused_over_three_steps=ratio("dequantize_gptq_fp16", "three_steps_fp16"),
                       fused_trivial_over_packed=ratio("dequantize_gptq_trivial_fp32", "dequantize_packed_fp32"))
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
        del sets, s0
        torch.cuda.empty_cache()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
