#!/usr/bin/env python3
"""Times of GPTQ's error-compensated rounding (AWQQuantizer.quantize_gptq, include/awq_hip.h
awq_gptq_round_block, csrc/awq_gptq_round.hip) on bf16 weights [N, K] with
`--tokens` correlated synthetic samples, 4-bit asymmetric, group size 128:

  * kernel: awq_gptq_round_block over every 128-column block of the weight, nothing between the
    launches (device events around the K / 128 launches; median of --rounds);
  * split: the solver's three parts on the same inputs, each between device events — the three
    Cholesky calls (torch.linalg), the kernel launches, the trailing GEMMs (addmm_) — and the wall
    time of one whole quantize_gptq call (H = X^T X, round-to-nearest and both output-error
    reports included);
  * torch loop: the same in-block loop spelled with torch ops on the GPU (per column: quotient,
    round, clamp, dequantize, error, rank-1 update of the block's later columns; group parameters
    by min / max at each group's first column), timed over --torch-blocks blocks and scaled to
    K / 128 blocks.  kernel_over_torch_loop is the ratio of the two per-block times.

  python scripts/gptq_round_bench.py [--rounds 5] [--tokens 512] [--torch-blocks 4] [--log FILE]
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

SHAPES = {"4096x4096": (4096, 4096), "4096x14336": (4096, 14336)}
GS, BITS, BLOCK = 128, 4, 128


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)            # ms


def torch_block(work, U, c0, err):
    """The in-block loop of one 128-column block with torch ops (fp32, asymmetric 4-bit)."""
    c1 = c0 + BLOCK
    W1, U1 = work[:, c0:c1], U[c0:c1, c0:c1]
    s = z = None
    for i in range(BLOCK):
        if i % GS == 0:
            g = W1[:, i:i + GS]
            mn, mx = g.amin(dim=1), g.amax(dim=1)
            s = ((mx - mn) / 15.0).clamp_min(1e-10).half().float()
            z = torch.round(-mn / s).clamp(0, 15)
        w = W1[:, i]
        q = (torch.round(w / s) + z).clamp(0, 15)
        e = (w - (q - z) * s) / U1[i, i]
        err[:, i] = e
        W1[:, i + 1:] -= e.unsqueeze(1) * U1[i, i + 1:].unsqueeze(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--torch-blocks", type=int, default=4)
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from awq_quantizer import _hip
    from awq_quantizer.quantization import AWQQuantizer
    from awq_quantizer.quantization.gptq_round import _factor
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    q = AWQQuantizer(bits=BITS, group_size=GS, symmetric=False, device="cuda:0", logger_level="ERROR")
    lines = []
    for name, (N, K) in SHAPES.items():
        g = torch.Generator(device=dev).manual_seed(N + K)
        x = (torch.randn(args.tokens, K, generator=g, device=dev) * torch.exp(torch.randn(K, generator=g, device=dev)))
        x = (x + 0.5 * x.roll(1, dims=1)).mul_(0.2).to(torch.bfloat16)         # neighbouring channels correlated
        w = (0.05 * torch.randn(N, K, generator=g, device=dev)).to(torch.bfloat16)
        H = x.float().t() @ x.float()
        U = None

        def chol():
            nonlocal U
            U = _factor(H, 0.01)
        chol()                                                               # warm (workspaces, code)
        t_chol = statistics.median(timed(chol) for _ in range(args.rounds))
        assert U is not None
        r = q._packed_outputs(w)
        r["qzeros"].zero_()
        blocks = [(c0, min(c0 + BLOCK, K)) for c0 in range(0, K, BLOCK)]
        errs = [torch.empty((N, c1 - c0), dtype=torch.float32, device=dev) for c0, c1 in blocks[:2]]
        base = w.float()
        work = base.clone()

        def kernels():
            for i, (c0, c1) in enumerate(blocks):
                _hip.gptq_round_block(work, U, GS, BITS, False, c0, c1 - c0, errs[i & 1], r["qweight"], r["qzeros"],
                                      r["scales"])
        kernels()
        t_kernel = []
        for _ in range(args.rounds):
            work.copy_(base)
            t_kernel.append(timed(kernels))

        def gemms():
            for i, (c0, c1) in enumerate(blocks):
                if c1 < K:
                    work[:, c1:].addmm_(errs[i & 1], U[c0:c1, c1:], alpha=-1.0)
        errs[0].normal_(std=1e-3)
        errs[1].normal_(std=1e-3)
        gemms()
        t_gemm = []
        for _ in range(args.rounds):
            work.copy_(base)
            t_gemm.append(timed(gemms))
        q.quantize_gptq(w, x)                                                # warm
        t_whole = []
        for _ in range(max(1, args.rounds // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = q.quantize_gptq(w, x)
            torch.cuda.synchronize()
            t_whole.append((time.perf_counter() - t0) * 1e3)
        nb = min(args.torch_blocks, len(blocks))
        err = torch.empty((N, BLOCK), dtype=torch.float32, device=dev)
        work.copy_(base)
        torch_block(work, U, 0, err)                                         # warm
        work.copy_(base)
        t_torch = timed(lambda: [torch_block(work, U, c0, err) for c0, _ in blocks[:nb]]) / nb
        med_kernel = statistics.median(t_kernel)
        out = {"weight": name, "N": N, "K": K, "tokens": args.tokens, "group_size": GS, "bits": BITS, "blocks": len(blocks),
               "kernel_ms": round(med_kernel, 3), "kernel_min_ms": round(min(t_kernel), 3),
               "kernel_max_ms": round(max(t_kernel), 3), "kernel_us_per_block": round(med_kernel * 1e3 / len(blocks), 1),
               "cholesky_ms": round(t_chol, 2), "gemm_ms": round(statistics.median(t_gemm), 3),
               "quantize_gptq_wall_ms": round(statistics.median(t_whole), 1),
               "torch_loop_us_per_block": round(t_torch * 1e3, 1), "torch_loop_ms_scaled": round(t_torch * len(blocks), 1),
               "kernel_over_torch_loop": round(med_kernel / len(blocks) / t_torch, 5),
               "loss_over_loss_rtn": round(res["rounding"]["loss"] / res["rounding"]["loss_rtn"], 4)}
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
        del H, U, work, base, res
        torch.cuda.empty_cache()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
