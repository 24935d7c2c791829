"""python -m awq_quantizer.rotate — a Hadamard-rotated copy of a Llama-layout model directory
(awq_quantizer/rotation.py).

  python -m awq_quantizer.rotate --model_id SRC --output_dir OUT [--seed 0] [--rotate_heads]
         [--dtype source|float32|bfloat16|float16]

OUT is an ordinary source checkpoint of the same function: safetensors shards, config.json (with
tie_word_embeddings false when lm_head had to be written), the tokenizer files, and rotation.json
(seed, h, m, k, heads, the tensors per operation).  calibrate, main, verify and evaluate run on it
unchanged.  Every argument error exits 1 before any device work.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import time
from typing import List, Optional

from .utils.logger import get_logger

SHARD_BYTES = 4 << 30
_TOKENIZER_FILES = ("tokenizer.json", "tokenizer.model", "tokenizer_config.json", "special_tokens_map.json",
                    "vocab.json", "merges.txt", "added_tokens.json", "generation_config.json")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="awq_quantizer.rotate", description="Hadamard rotation of a model directory")
    p.add_argument("--model_id", type=str, required=True, help="Model directory (config.json + safetensors)")
    p.add_argument("--output_dir", type=str, required=True, help="Directory to write the rotated model to")
    p.add_argument("--seed", type=int, default=0, help="Seed of the sign vector d")
    p.add_argument("--rotate_heads", action="store_true", help="Also rotate every head of v_proj / o_proj (R2)")
    p.add_argument("--dtype", type=str, default="source", choices=["source", "float32", "bfloat16", "float16"],
                   help="Dtype the tensors are written in")
    p.add_argument("--device", type=str, default="cuda", help="The GPU to run on (there is no CPU path)")
    p.add_argument("--log_level", type=str, default="INFO", choices=["DEBUG", "INFO", "WARNING", "ERROR", "CRITICAL"])
    return p


def main(argv: Optional[List[str]] = None) -> int:
    try:
        args = build_parser().parse_args(argv)
    except SystemExit as e:
        return 0 if e.code in (0, None) else 1
    logger = get_logger(name="awq_rotate", level=args.log_level)
    try:
        import torch
        from .model_loading.safetensors_loader import SafetensorsLoader
        from .rotation import plan_rotation
        if not os.path.isdir(args.model_id):
            raise ValueError(f"--model_id: {args.model_id} is not a directory")
        if os.path.abspath(args.model_id) == os.path.abspath(args.output_dir):
            raise ValueError("--output_dir must differ from --model_id")
        with open(os.path.join(args.model_id, "config.json")) as f:
            config = json.load(f)
        loader = SafetensorsLoader(args.model_id, logger_level="WARNING")
        index = {i.name: i for i in loader.tensor_index()}
        plan = plan_rotation({n: i.shape for n, i in index.items()}, config)
    except (ValueError, OSError, KeyError) as e:
        logger.error(str(e))
        return 1
    try:
        from . import _hip
        from .output import save_safetensors
        from .rotation import apply_op, rotation_signs
        device = torch.device(args.device)
        _hip.require_device(device)
        t0 = time.time()
        os.makedirs(args.output_dir, exist_ok=True)
        d = rotation_signs(plan.h, args.seed).to(device)
        dtype = None if args.dtype == "source" else getattr(torch, args.dtype)

        def read(name):
            t = loader.read(index[name])
            return t.to(dtype) if dtype is not None and t.is_floating_point() else t

        shards, shard, size, total = [], {}, 0, 0          # shards: the names of each written file's tensors

        def flush():
            # (written under a rank-free temporary name: the final names carry the number of shards)
            save_safetensors(shard, os.path.join(args.output_dir, f".shard_{len(shards):05d}.safetensors"))
            shards.append(list(shard))

        for name, op in plan.ops.items():
            out = apply_op(op, read(op.source or name), plan, d, read(op.norm) if op.norm else None,
                           args.rotate_heads, device)
            nb = out.numel() * out.element_size()
            if shard and size + nb > SHARD_BYTES:
                flush()
                shard, size = {}, 0
            shard[name], size, total = out, size + nb, total + nb
        flush()
        weight_map = {}
        for i, names in enumerate(shards):
            fname = "model.safetensors" if len(shards) == 1 else f"model-{i + 1:05d}-of-{len(shards):05d}.safetensors"
            os.replace(os.path.join(args.output_dir, f".shard_{i:05d}.safetensors"), os.path.join(args.output_dir, fname))
            weight_map.update({n: fname for n in names})
        if len(shards) > 1:
            with open(os.path.join(args.output_dir, "model.safetensors.index.json"), "w") as f:
                json.dump({"metadata": {"total_size": total}, "weight_map": weight_map}, f, indent=2)
        if plan.tied:
            config["tie_word_embeddings"] = False
        if dtype is not None and ("torch_dtype" in config or "dtype" in config):
            config["torch_dtype" if "torch_dtype" in config else "dtype"] = args.dtype
        with open(os.path.join(args.output_dir, "config.json"), "w") as f:
            json.dump(config, f, indent=2)
        for fn in _TOKENIZER_FILES:
            if os.path.isfile(os.path.join(args.model_id, fn)):
                shutil.copyfile(os.path.join(args.model_id, fn), os.path.join(args.output_dir, fn))
        with open(os.path.join(args.output_dir, "rotation.json"), "w") as f:
            json.dump({"seed": args.seed, "h": plan.h, "m": plan.m, "k": plan.k, "head_dim": plan.head_dim,
                       "heads": bool(args.rotate_heads), "dtype": args.dtype, "tied_lm_head_written": plan.tied,
                       "tensors": plan.by_operation(args.rotate_heads)}, f, indent=2)
        loader.close()
    except Exception as e:  # noqa: BLE001
        logger.error(f"Rotation failed: {e}")
        return 1
    logger.info(f"Wrote {len(plan.ops)} tensors ({total} bytes, {len(shards)} shard(s)) to {args.output_dir}")
    logger.info("metrics " + json.dumps({"tensors": len(plan.ops), "bytes": total, "seconds": round(time.time() - t0, 4)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
