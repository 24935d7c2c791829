#!/usr/bin/env python3
"""One evaluate-shaped run on a synthetic Llama-3-8B-shaped model, split by HIP events into its
phases: the decoder blocks of both models (calibration/forward.py run_decoder, statistics off), the
tail's final norms and head GEMMs, and awq_logit_compare.  Random bf16 weights made on the device
by a loader object (nothing is written to disk), 32 x 512 tokens by default, the second model the
first plus noise.  It shows the size of the new kernel's share of an evaluation; the figures of the
kernel itself are scripts/logit_compare_bench.py's.  One JSON line.

  python scripts/evaluate_e2e_bench.py [--n 32 --seq 512 --layers 32 --batch-tokens 8192]
"""
import argparse
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "awq-converter_amd")]
import torch  # noqa: E402

from awq_quantizer import evaluation as ev  # noqa: E402
from awq_quantizer.calibration.forward import parse_config, run_decoder  # noqa: E402
from awq_quantizer.model_loading.safetensors_loader import TensorInfo  # noqa: E402

LLAMA3_8B = {"model_type": "llama", "hidden_size": 4096, "intermediate_size": 14336, "num_hidden_layers": 32,
             "num_attention_heads": 32, "num_key_value_heads": 8, "vocab_size": 128256, "rms_norm_eps": 1e-5,
             "rope_theta": 500000.0, "max_position_embeddings": 8192, "hidden_act": "silu"}


class RandomLoader:
    """tensor_index() / read() of a model that exists only as shapes: N(0, 0.02^2) weights (norms 1 + that),
    seeded by the tensor's name, plus `noise` times a second draw (the 'quantized' model)."""

    def __init__(self, cfg, device, noise=0.0):
        H, I, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
        kv = H // cfg["num_attention_heads"] * cfg["num_key_value_heads"]
        shapes = {"model.embed_tokens.weight": (V, H), "model.norm.weight": (H,), "lm_head.weight": (V, H)}
        for i in range(cfg["num_hidden_layers"]):
            p = f"model.layers.{i}."
            shapes.update({p + "input_layernorm.weight": (H,), p + "post_attention_layernorm.weight": (H,),
                           p + "self_attn.q_proj.weight": (H, H), p + "self_attn.k_proj.weight": (kv, H),
                           p + "self_attn.v_proj.weight": (kv, H), p + "self_attn.o_proj.weight": (H, H),
                           p + "mlp.gate_proj.weight": (I, H), p + "mlp.up_proj.weight": (I, H),
                           p + "mlp.down_proj.weight": (H, I)})
        self._index = [TensorInfo(n, None, torch.bfloat16, s) for n, s in shapes.items()]
        self.device, self.noise = device, noise

    def tensor_index(self):
        return self._index

    def read(self, info):
        g = torch.Generator(device=self.device).manual_seed(zlib.crc32(info.name.encode()))
        w = torch.randn(info.shape, device=self.device, generator=g) * 0.02
        if len(info.shape) == 1:
            w += 1.0
        if self.noise:
            w += torch.randn(info.shape, device=self.device, generator=g) * (0.02 * self.noise)
        return w.bfloat16()


class TimedOps(ev.HipEvalOps):
    def __init__(self, device):
        super().__init__(device)
        self.events = []

    def logit_compare(self, ref, q, targets):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = super().logit_compare(ref, q, targets)
        b.record()
        self.events.append((a, b))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batch-tokens", type=int, default=8192)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    raw = dict(LLAMA3_8B, num_hidden_layers=args.layers)
    cfg = parse_config(raw, seq_len=args.seq)
    ids = torch.randint(0, raw["vocab_size"], (args.n, args.seq), generator=torch.Generator().manual_seed(0))
    ops = TimedOps(dev)
    loaders = [RandomLoader(raw, dev), RandomLoader(raw, dev, noise=0.05)]
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    with torch.no_grad():
        marks[0].record()
        hiddens = []
        for ld in loaders:
            got = {}
            run_decoder(ld, cfg, ids, torch.bfloat16, dev, ops, batch_tokens=args.batch_tokens, stats=False, hidden_out=got)
            hiddens.append(got["hidden"])
        marks[1].record()
        targets = ev.shifted_targets(ids).to(dev)
        per = ev._tail(cfg, loaders, hiddens, targets, torch.bfloat16, dev, ops, args.batch_tokens)
        marks[2].record()
    torch.cuda.synchronize()
    compare = sum(a.elapsed_time(b) for a, b in ops.events)
    blocks, tail = marks[0].elapsed_time(marks[1]), marks[1].elapsed_time(marks[2])
    r = ev.aggregate(per, targets)
    print(json.dumps({"model": "synthetic Llama-3-8B shape, random bf16 weights made on the device", "layers": args.layers,
                      "tokens": args.n * args.seq, "batch_tokens": args.batch_tokens, "models": 2,
                      "blocks_ms": round(blocks, 2), "tail_ms": round(tail, 2), "compare_ms": round(compare, 3),
                      "head_and_norm_ms": round(tail - compare, 2), "compare_calls": len(ops.events),
                      "compare_share_of_total": round(compare / (blocks + tail), 5),
                      "ppl_ref": r["ppl_ref"], "kl_mean": r["kl_mean"], "nonfinite_rows": r["nonfinite_rows"]}))


if __name__ == "__main__":
    main()
