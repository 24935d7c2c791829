#!/usr/bin/env python3
"""The calibration pass' three fused entries (awq_act_stats_accum, awq_rmsnorm_stats,
awq_swiglu_stats) against (a) the torch composition each replaces, as a forward hook would write
it, and (b) awq_stream_copy moving the entry's algorithmic bytes (the memory yardstick) —
interleaved in one process (HIP events, `--rounds` rounds of windows of at least `--window-ms`
each, medians with min / max).  Every case cycles over enough buffer sets that no launch finds its
input in the Infinity Cache; what one launch itself re-reads (the norm reads x twice) is its own.

Default shapes: Llama-3-8B's activations at a micro-batch of 8192 tokens, bf16, K = 4096 and 14336.
Algorithmic bytes (N = tokens * K * element size): accum reads N; the norm reads N and writes N;
SwiGLU reads 2N and writes N.  The copy moves the same total (it reads half and writes half).
One JSON line per (entry, K): *_us medians, `fused_over_torch` = torch time / fused time,
`fused_over_copy_rate` = copy time / fused time (1.0: the entry streams its bytes as fast as a copy).

  python scripts/calibrate_bench.py [--tokens 8192] [--K 4096,14336] [--dtype bf16] | tee profiles/calibrate_bench.log
  python scripts/calibrate_bench.py --block     one synthetic Llama-3-8B block, 128 x 512 tokens (for
                                                a kernel trace: the split of block time by kernel)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "awq-converter_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from awq_quantizer import _hip  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
EPS = 1e-5


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def torch_stats(v):
    """Column sums of |v| and v^2 as a forward hook would take them (fp32 accumulation)."""
    f = v.float()
    return f.abs().sum(0), f.pow(2).sum(0)


def bench_entry(entry, T, K, dtype, rounds, window_ms, footprint):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(T + K)
    esize = torch.empty((), dtype=dtype).element_size()
    N = T * K * esize
    n_in = {"accum": 1, "rmsnorm": 1, "swiglu": 2}[entry]
    alg = {"accum": N, "rmsnorm": 2 * N, "swiglu": 3 * N}[entry]
    reps = max(2, -(-footprint // (n_in * N)))
    if entry == "swiglu":        # gate | up: the two column halves of one fused GEMM output
        sets = [torch.randn(T, 2 * K, device=dev, generator=g).to(dtype) for _ in range(reps)]
    else:
        sets = [torch.randn(T, K, device=dev, generator=g).to(dtype) for _ in range(reps)]
    w = (1.0 + 0.2 * torch.randn(K, device=dev, generator=g)).to(dtype)
    out = torch.empty(T, K, dtype=dtype, device=dev)
    acc_a = torch.zeros(K, dtype=torch.float64, device=dev)
    acc_s = torch.zeros(K, dtype=torch.float64, device=dev)
    work = torch.empty(_hip.calib_work_size(T, K, norm=True), dtype=torch.float64, device=dev)
    copy_src = [s.view(-1)[: alg // 2 // esize] for s in sets]      # the copy reads half, writes half
    copy_dst = torch.empty(alg // 2 // esize, dtype=dtype, device=dev)
    stream = _hip.stream_ptr(dev)
    turn = {"i": 0}

    def pick(pool):
        turn["i"] = (turn["i"] + 1) % reps
        return pool[turn["i"]]

    def fused():
        x = pick(sets)
        if entry == "accum":
            _hip.act_stats_accum(x, 0, acc_a, acc_s, work=work)
        elif entry == "rmsnorm":
            _hip.rmsnorm_stats(x, w, EPS, 0, acc_a, acc_s, out=out, work=work)
        else:
            _hip.swiglu_stats(x[:, :K], x[:, K:], 0, acc_a, acc_s, out=out, work=work)

    def composed():
        x = pick(sets)
        if entry == "accum":
            return torch_stats(x)
        if entry == "rmsnorm":
            xf = x.float()
            h = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS)).to(dtype)
            return torch_stats(w * h)
        return torch_stats(F.silu(x[:, :K]) * x[:, K:])

    def copy():
        _hip.stream_copy(pick(copy_src), copy_dst, stream)

    cases = {"fused": fused, "torch": composed, "copy": copy}
    iters = {}
    for name, fn in cases.items():
        fn()
        torch.cuda.synchronize()
        iters[name] = max(3, int(window_ms * 1e3 / max(timed(fn, 3), 1.0)) + 1)
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for name, fn in cases.items():
            times[name].append(timed(fn, iters[name]))
    us = {k: statistics.median(v) for k, v in times.items()}
    r = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
         "entry": entry, "tokens": T, "K": K, "dtype": str(dtype).split(".")[-1], "algorithmic_bytes": alg,
         "buffer_sets_cycled": reps, "launches_per_window": iters}
    for k in cases:
        r[k + "_us"] = round(us[k], 1)
        r[k + "_us_min_max"] = [round(min(times[k]), 1), round(max(times[k]), 1)]
    r["fused_TBps"] = round(alg / us["fused"] * 1e-6, 3)
    r["copy_TBps"] = round(alg / us["copy"] * 1e-6, 3)
    r["fused_over_torch"] = round(us["torch"] / us["fused"], 3)
    r["fused_over_copy_rate"] = round(us["copy"] / us["fused"], 3)
    return r


def synthetic_block(n_seq, seq, dtype):
    """One decoder block at Llama-3-8B shapes with random weights through the product's driver."""
    from awq_quantizer.calibration import DecoderConfig, HipOps, run_decoder

    class Info:
        def __init__(self, name, t):
            self.name, self.tensor, self.dtype, self.shape = name, t, t.dtype, tuple(t.shape)

    class Loader:
        def __init__(self, tensors):
            self.infos = [Info(k, v) for k, v in tensors.items()]

        def tensor_index(self):
            return self.infos

        def read(self, info):
            return info.tensor

    H, I, nh, nkv, hd, V = 4096, 14336, 32, 8, 128, 1024
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.02).to(dtype)
    p = "model.layers.0."
    tensors = {"model.embed_tokens.weight": torch.randn(V, H, generator=g).to(dtype),
               p + "input_layernorm.weight": torch.ones(H, dtype=dtype),
               p + "post_attention_layernorm.weight": torch.ones(H, dtype=dtype),
               p + "self_attn.q_proj.weight": rnd(nh * hd, H), p + "self_attn.k_proj.weight": rnd(nkv * hd, H),
               p + "self_attn.v_proj.weight": rnd(nkv * hd, H), p + "self_attn.o_proj.weight": rnd(H, nh * hd),
               p + "mlp.gate_proj.weight": rnd(I, H), p + "mlp.up_proj.weight": rnd(I, H),
               p + "mlp.down_proj.weight": rnd(H, I)}
    cfg = DecoderConfig("llama", H, 1, nh, nkv, hd, V, 8192, 1e-5, 500000.0, "default", {}, None, True)
    ids = torch.randint(0, V, (n_seq, seq), generator=g)
    dev = torch.device("cuda", 0)
    ops = HipOps(dev)
    run_decoder(Loader(tensors), cfg, ids, dtype, dev, ops)          # warm-up (library handles, kernels' first use)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    stats = run_decoder(Loader(tensors), cfg, ids, dtype, dev, ops)
    b.record()
    b.synchronize()
    print(json.dumps({"block": "llama-3-8b shapes", "tokens": n_seq * seq, "dtype": str(dtype).split(".")[-1],
                      "wall_ms_incl_h2d": round(a.elapsed_time(b), 2), "weights": len(stats)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--K", default="4096,14336")
    ap.add_argument("--dtype", default="bf16", choices=sorted(DTYPES))
    ap.add_argument("--entries", default="accum,rmsnorm,swiglu")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0, help="least length of a timed window")
    ap.add_argument("--footprint-mib", type=int, default=1024,
                    help="inputs cycled through before a buffer is read again")
    ap.add_argument("--block", action="store_true", help="run one synthetic Llama-3-8B block instead")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("calibrate_bench: needs a GPU (no CPU fallback; a CPU timing would say nothing)")
    _hip.require_device(torch.device("cuda", 0))
    if a.block:
        synthetic_block(128, 512, DTYPES[a.dtype])
        return
    for K in (int(v) for v in a.K.split(",")):
        for entry in a.entries.split(","):
            print(json.dumps(bench_entry(entry, a.tokens, K, DTYPES[a.dtype], a.rounds, a.window_ms,
                                         a.footprint_mib << 20)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
