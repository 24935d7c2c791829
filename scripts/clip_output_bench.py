#!/usr/bin/env python3
"""awq_quantize_clip_output (the clip search with the token-sample loss) against the three things it
is quoted against, interleaved in one process on the same tensors (HIP events, `--rounds` rounds of
windows of at least `--window-ms` each, medians and min / max; every case cycles over enough copies
of the weights that no launch finds them in the Infinity Cache):
  * torch_published: a torch restatement of the published per-group loss on the GPU in fp32 — for
    every candidate the shrunk range, scale and zero point per group, the dequantized error, one
    einsum [rows, G, L] x [T, G, L] -> [rows, G, T] in row batches, squared and summed over tokens,
    a running minimum (the shape of AutoAWQ's _compute_best_clip; its roundings are not restated);
  * bf16_matmul: one bf16 torch.matmul of the same (N, K, T): the library's rate for ONE MFMA per
    k-step; the kernel issues two per candidate, so its work is quoted as a fraction of
    2 * n_candidates times that matmul;
  * diag_clip: awq_quantize_clip_scaled, today's diagonal clip loss — what the better objective costs.
Default shapes: Llama-3-8B's MLP up / down projections, bf16, gs 128, 4-bit, T = 512, grid 20 with
10 candidates.  One JSON line per shape.

  python scripts/clip_output_bench.py [--shapes 14336x4096,4096x14336] [--tokens 512]
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


def torch_published(w, s, x, L, bits, n_grid, n_cand, row_batch):
    """-> (best index [N, G], its loss [N, G]) of the asymmetric per-group clip search in fp32"""
    N, K = w.shape
    G, T, qmax = K // L, x.shape[0], float((1 << bits) - 1)
    xg = x.float().view(T, G, L)
    sg = s.view(1, G, L)
    best_i = torch.zeros((N, G), dtype=torch.int32, device=w.device)
    best_l = torch.full((N, G), float("inf"), dtype=torch.float32, device=w.device)
    for r0 in range(0, N, row_batch):
        wb = w[r0:r0 + row_batch].float().view(-1, G, L)
        ws = wb * sg
        mn, mx = ws.amin(dim=-1, keepdim=True), ws.amax(dim=-1, keepdim=True)
        for i in range(n_cand):
            a = (n_grid - i) / n_grid
            scale = ((mx - mn) * (a / qmax)).clamp_min(1e-10)
            z = (-(mn * a) / scale).round().clamp(0, qmax)
            q = (ws / scale + z).round().clamp(0, qmax)
            d = (q - z) * scale / sg - wb
            loss = torch.einsum("ngk,tgk->ngt", d, xg).square().sum(dim=-1)
            take = loss < best_l[r0:r0 + row_batch]
            best_l[r0:r0 + row_batch] = torch.where(take, loss, best_l[r0:r0 + row_batch])
            best_i[r0:r0 + row_batch] = torch.where(take, torch.full_like(best_i[r0:r0 + row_batch], i),
                                                    best_i[r0:r0 + row_batch])
    return best_i, best_l


def bench_shape(N, K, T, L, bits, n_grid, n_cand, rounds, window_ms, footprint, row_batch):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(N + K)
    q = AWQQuantizer(bits=bits, group_size=L, symmetric=False, device="cuda:0", logger_level="ERROR")
    reps = max(1, -(-footprint // (N * K * 2)))
    ws = [(torch.randn(N, K, device=dev, generator=g) * 0.02).bfloat16() for _ in range(reps)]
    x = (torch.randn(T, K, device=dev, generator=g) * (0.25 + 4 * torch.rand(K, device=dev, generator=g) ** 3)).bfloat16()
    s = torch.exp((torch.rand(K, device=dev, generator=g) * 2 - 1) * 1.386).float()
    rs = _hip.act_recip_table(s.reshape(1, K)).reshape(K)
    x_sq = (x.float() ** 2).mean(dim=0)
    r = q._packed_outputs(ws[0])
    G = K // L
    idx = torch.empty(N * G, dtype=torch.int32, device=dev)
    idx_d = torch.empty(N * G, dtype=torch.int32, device=dev)
    loss = torch.empty((2, N * G), dtype=torch.float32, device=dev)
    loss_d = torch.empty((2, N * G), dtype=torch.float32, device=dev)
    turn = {"i": 0}
    keep = {}

    def pick():
        turn["i"] = (turn["i"] + 1) % reps
        return ws[turn["i"]]

    def clip_output():
        _hip.quantize_clip_output(pick(), s, x, L, bits, False, n_grid, n_cand, rscale=rs, qweight=r["qweight"],
                                  qzeros=r["qzeros"], scales=r["scales"], best_idx=idx, group_loss=loss)

    def diag_clip():
        _hip.quantize_clip_scaled(pick(), s, x_sq, L, bits, False, n_grid, n_cand, rscale=rs, qweight=r["qweight"],
                                  qzeros=r["qzeros"], scales=r["scales"], best_idx=idx_d, group_loss=loss_d)

    def published():
        keep["p"] = torch_published(pick(), s, x, L, bits, n_grid, n_cand, row_batch)

    def bf16_matmul():
        keep["m"] = torch.matmul(pick(), x.t())

    cases = {"clip_output": clip_output, "torch_published": published, "bf16_matmul": bf16_matmul, "diag_clip": diag_clip}
    iters = {}
    for name, fn in cases.items():          # warm-up of every case on this shape, and its window length
        fn()
        torch.cuda.synchronize()
        iters[name] = max(3, int(window_ms * 1e3 / max(timed(fn, 3), 1.0)) + 1)
    turn["i"] = reps - 1                    # the three searches on copy 0, side by side
    clip_output()
    turn["i"] = reps - 1
    published()
    turn["i"] = reps - 1
    diag_clip()
    # what the diagonal clip's winners cost in the output loss: every candidate's loss of copy 0
    cand = torch.empty((n_cand, N * G), dtype=torch.float32, device=dev)
    _hip.quantize_clip_output(ws[0], s, x, L, bits, False, n_grid, n_cand, rscale=rs, cand_loss=cand)
    torch.cuda.synchronize()
    both = loss.double().sum(dim=1)
    diag_after = cand.gather(0, idx_d.long().reshape(1, -1)).double().sum()
    agree = {"winners_equal_torch_published": float((idx.view(N, G) == keep["p"][0]).float().mean()),
             "winners_equal_diag_clip": float((idx == idx_d).float().mean()),
             "output_loss_after_over_before": float(both[1] / both[0]),
             "output_loss_after_over_before_with_diag_clip": float(diag_after / both[0]),
             "torch_published_loss_after": float(keep["p"][1].double().sum()), "loss_after": float(both[1]),
             "clipped_fraction": float((idx != 0).float().mean())}
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for name, fn in cases.items():
            times[name].append(timed(fn, iters[name]))
    us = {k: statistics.median(v) for k, v in times.items()}
    flop = 2.0 * N * K * T
    out = {"N": N, "K": K, "T": T, "group_size": L, "bits": bits, "dtype": "bf16", "n_grid": n_grid,
           "n_candidates": n_cand, "weight_copies_cycled": reps, "launches_per_window": iters}
    for k in cases:
        out[k + "_us"] = round(us[k], 1)
        out[k + "_us_min_max"] = [round(min(times[k]), 1), round(max(times[k]), 1)]
    out.update(speedup_over_torch_published=round(us["torch_published"] / us["clip_output"], 2),
               bf16_matmul_TFLOPs=round(flop / us["bf16_matmul"] / 1e6, 1),
               clip_output_mfma_TFLOPs=round(2 * n_cand * flop / us["clip_output"] / 1e6, 1),
               frac_of_2n_matmuls=round(2 * n_cand * us["bf16_matmul"] / us["clip_output"], 3),
               cost_over_diag_clip=round(us["clip_output"] / us["diag_clip"], 1), searches=agree)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="14336x4096,4096x14336")
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--group-size", type=int, default=128)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--candidates", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0, help="least length of a timed window")
    ap.add_argument("--footprint-mib", type=int, default=1024,
                    help="weights cycled through before a tensor is read again (0: one copy, cache-warm)")
    ap.add_argument("--row-batch", type=int, default=1024, help="rows per einsum of the torch restatement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_output_bench: needs a GPU (no CPU fallback; a CPU timing would say nothing)")
    _hip.require_device(torch.device("cuda", 0))
    for sh in [v for v in a.shapes.split(",") if v]:
        N, K = (int(v) for v in sh.lower().split("x"))
        print(json.dumps(bench_shape(N, K, a.tokens, a.group_size, a.bits, a.grid, a.candidates, a.rounds, a.window_ms,
                                     a.footprint_mib << 20, a.row_batch)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
