#!/usr/bin/env python3
"""awq_quantize_clip_scaled (the activation-aware clip search) against the two things it is
quoted against, interleaved in one process on the same tensors (HIP events, `--rounds` rounds of
windows of at least `--window-ms` each, medians; every case cycles over enough copies of the
tensor that no launch finds its input in the Infinity Cache):
  * composed: the path available without it — awq_apply_input_scale into a copy, then
    awq_quantize_search on the copy with the same grid.  Its search is UNWEIGHTED (plain squared
    error of the scaled weights): a cost yardstick, not the same result;
  * rtn: awq_quantize_groups_scaled, the one-pass RTN of W diag(s) the clip search replaces.
Synthetic inputs: N(0, 0.02) weights, s log-uniform in [1/4, 4], x_sq = u^4 + 1e-4.  Also the
quality figure on those inputs: the layer loss after / before clipping and the clipped fraction.
Default shapes: Llama-3-8B's MLP down / up projections and lm_head, bf16, gs 128, 4-bit
asymmetric, grid 20, 10 candidates.  One JSON line per shape.

  python scripts/act_clip_bench.py [--shapes 14336x4096,4096x14336,128256x4096]
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
from awq_quantizer.quantization import AWQQuantizer  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def bench_shape(rows, K, L, bits, n_grid, n_cand, rounds, window_ms, footprint):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(rows + K)
    q = AWQQuantizer(bits=bits, group_size=L, symmetric=False, device="cuda:0", logger_level="ERROR")
    n, G = rows * K, K // L
    ng = rows * G
    reps = max(1, -(-footprint // (n * 2)))
    ws = [(torch.randn(rows, K, device=dev, generator=g) * 0.02).bfloat16() for _ in range(reps)]
    s = torch.exp2(torch.rand(K, device=dev, generator=g) * 4 - 2).float()
    xs = (torch.rand(K, device=dev, generator=g) ** 4 + 1e-4).float()
    rs = _hip.act_recip_table(s.reshape(1, K)).reshape(K)
    out = q._packed_outputs(ws[0])
    best = torch.empty(ng, dtype=torch.int32, device=dev)
    loss = torch.empty((2, ng), dtype=torch.float32, device=dev)
    copy = torch.empty_like(ws[0])
    lib = _hip.load_library()
    turn = {"i": 0}

    def pick():
        turn["i"] = (turn["i"] + 1) % reps
        return ws[turn["i"]]

    def clip():
        _hip.quantize_clip_scaled(pick(), s, xs, L, bits, False, n_grid, n_cand, rscale=rs, qweight=out["qweight"],
                                  qzeros=out["qzeros"], scales=out["scales"], best_idx=best, group_loss=loss)

    def clip_ieee():
        _hip.quantize_clip_scaled(pick(), s, xs, L, bits, False, n_grid, n_cand, rscale=None, qweight=out["qweight"],
                                  qzeros=out["qzeros"], scales=out["scales"], best_idx=best, group_loss=loss)

    def composed():
        w = pick()
        _hip.check(lib.awq_apply_input_scale(_hip.ptr(w), _hip.AWQ_DTYPE[w.dtype], rows, K, _hip.ptr(s),
                                             _hip.ptr(copy), _hip._stream(w)), "awq_apply_input_scale")
        _hip.quantize_search(copy, rows, K, L, bits, False, n_grid, n_cand, qweight=out["qweight"],
                             qzeros=out["qzeros"], scales=out["scales"])

    def search_only():
        _hip.quantize_search(pick(), rows, K, L, bits, False, n_grid, n_cand, qweight=out["qweight"],
                             qzeros=out["qzeros"], scales=out["scales"])

    def rtn():
        _hip.quantize_groups_scaled(pick(), s, L, bits, False, qweight=out["qweight"], qzeros=out["qzeros"],
                                    scales=out["scales"])

    cases = {"clip": clip, "clip_ieee": clip_ieee, "composed": composed, "search_only": search_only, "rtn": rtn}
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
    # the quality figure, on copy 0
    turn["i"] = reps - 1
    clip()
    tot, _, _ = _hip.act_search_select(loss, s.reshape(1, K).expand(2, K).contiguous())
    tot = tot.cpu().tolist()
    frac = float((best != 0).float().mean().item())
    r = {"rows": rows, "K": K, "group_size": L, "bits": bits, "dtype": "bf16", "n_grid": n_grid,
         "n_candidates": n_cand, "tensor_copies_cycled": reps, "launches_per_window": iters}
    for k in cases:
        r[k + "_us"] = round(us[k], 1)
        r[k + "_us_min_max"] = [round(min(times[k]), 1), round(max(times[k]), 1)]
    r.update({"clip_over_composed": round(us["clip"] / us["composed"], 3),
              "clip_over_search_only": round(us["clip"] / us["search_only"], 3),
              "clip_over_rtn": round(us["clip"] / us["rtn"], 2),
              "ns_per_candidate_element": round(us["clip"] * 1e3 / (n * n_cand), 5),
              "loss_before": tot[0], "loss_after": tot[1], "loss_after_over_before": round(tot[1] / tot[0], 4),
              "clipped_fraction": round(frac, 4)})
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="14336x4096,4096x14336,128256x4096")
    ap.add_argument("--group-size", type=int, default=128)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--candidates", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0, help="least length of a timed window")
    ap.add_argument("--footprint-mib", type=int, default=1024,
                    help="weights cycled through before a tensor is read again (0: one copy, cache-warm)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("act_clip_bench: needs a GPU (no CPU fallback; a CPU timing would say nothing)")
    _hip.require_device(torch.device("cuda", 0))
    for sh in a.shapes.split(","):
        rows, K = (int(v) for v in sh.lower().split("x"))
        r = bench_shape(rows, K, a.group_size, a.bits, a.grid, a.candidates, a.rounds, a.window_ms,
                        a.footprint_mib << 20)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
