"""python -m awq_quantizer.evaluate — perplexity of a model directory on token ids and, with a
directory main wrote, of the quantized model, the KL divergence between the two and their top-1
agreement, on the GPU (awq_quantizer/evaluation).

  python -m awq_quantizer.evaluate --model_id DIR --input_ids ids.safetensors
  python -m awq_quantizer.evaluate --model_id DIR --quantized_dir OUT --text_file corpus.txt \
         --n_samples 32 --seq_len 512 --report eval.json --max_ppl_ratio 1.05 --max_kl 0.05

The token-id and text options are calibrate's.  One JSON line of the aggregates goes to stdout;
--report also writes them with the arguments.  Returns 0, or 1 on any refusal (all argument and
config.json refusals happen before the model is read), on nonfinite_rows > 0, and when ppl_ratio
exceeds --max_ppl_ratio or kl_mean exceeds --max_kl (which need --quantized_dir).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from typing import List, Optional

from .utils.logger import get_logger


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="awq_quantizer.evaluate",
                                description="Perplexity, KL divergence and top-1 agreement of a written checkpoint")
    p.add_argument("--model_id", type=str, required=True, help="Source model directory (config.json + safetensors)")
    p.add_argument("--quantized_dir", type=str, default=None,
                   help="A directory main wrote (reference / packed / autoawq); without it only the source is scored")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--input_ids", type=str, help="safetensors with input_ids int64 [n, seq], or a .npy")
    src.add_argument("--text_file", type=str, help="Plain text, tokenised with the model's tokenizer.json")
    p.add_argument("--n_samples", type=int, default=128, help="--text_file: sequences kept")
    p.add_argument("--seq_len", type=int, default=512, help="--text_file: tokens per sequence")
    p.add_argument("--compute_dtype", type=str, default=None, choices=["bfloat16", "float16", "float32"],
                   help="Dtype of the forward (default: the checkpoint's)")
    p.add_argument("--batch_tokens", type=int, default=8192, help="Tokens per micro-batch and per head chunk")
    p.add_argument("--report", type=str, default=None, help="Also write the aggregates and the arguments (JSON)")
    p.add_argument("--max_ppl_ratio", type=float, default=None, help="Return 1 when ppl_q / ppl_ref exceeds this")
    p.add_argument("--max_kl", type=float, default=None, help="Return 1 when the mean KL divergence exceeds this")
    p.add_argument("--device", type=str, default="cuda", help="The GPU to run on (there is no CPU path)")
    p.add_argument("--log_level", type=str, default="INFO", choices=["DEBUG", "INFO", "WARNING", "ERROR", "CRITICAL"])
    return p


def check_args(args) -> Optional[str]:
    """The flag rules, host only; the first violated one as a message."""
    if args.batch_tokens <= 0:
        return "--batch_tokens must be positive"
    for flag in ("max_ppl_ratio", "max_kl"):
        v = getattr(args, flag)
        if v is not None and args.quantized_dir is None:
            return f"--{flag} needs --quantized_dir"
        if v is not None and (math.isnan(v) or v < 0):
            return f"--{flag} must be a non-negative number"
    if not os.path.isdir(args.model_id):
        return f"--model_id: {args.model_id} is not a directory"
    if args.quantized_dir is not None and not os.path.isdir(args.quantized_dir):
        return f"--quantized_dir: {args.quantized_dir} is not a directory"
    return None


def gates(result: dict, args) -> List[str]:
    """What makes a finished evaluation return 1."""
    out = []
    if result.get("nonfinite_rows", 0) > 0:
        out.append(f"{result['nonfinite_rows']} rows of logits hold a NaN or an infinity")
    if args.max_ppl_ratio is not None and not result["ppl_ratio"] <= args.max_ppl_ratio:
        out.append(f"ppl_ratio {result['ppl_ratio']:.6g} exceeds --max_ppl_ratio {args.max_ppl_ratio:g}")
    if args.max_kl is not None and not result["kl_mean"] <= args.max_kl:
        out.append(f"kl_mean {result['kl_mean']:.6g} exceeds --max_kl {args.max_kl:g}")
    return out


def main(argv: Optional[List[str]] = None, evaluate_fn=None) -> int:
    """evaluate_fn(model_dir, ids, **kw) -> aggregates; default: evaluation.evaluate_model."""
    try:
        args = build_parser().parse_args(argv)
    except SystemExit as e:            # argparse exits 2; this tool's argument errors are all 1
        return 0 if e.code in (0, None) else 1
    logger = get_logger(name="awq_evaluate", level=args.log_level)
    try:
        from .calibrate import load_ids
        from .calibration import parse_config, read_config
        why = check_args(args)
        if why:
            raise ValueError(why)
        cfg = read_config(args.model_id)
        parse_config(cfg)                      # model type, rope type: before the ids are read
        ids = load_ids(args)
        parse_config(cfg, seq_len=ids.shape[1], max_id=int(ids.max()))
    except (ValueError, OSError) as e:
        logger.error(str(e))
        return 1
    try:
        if evaluate_fn is None:
            from .evaluation import evaluate_model as evaluate_fn
        result = evaluate_fn(args.model_id, ids, quantized_dir=args.quantized_dir, compute_dtype=args.compute_dtype,
                             batch_tokens=args.batch_tokens, device=args.device, logger=logger)
    except Exception as e:  # noqa: BLE001
        logger.error(f"Evaluation failed: {e}")
        return 1
    print(json.dumps(result), flush=True)
    failed = gates(result, args)
    if args.report:
        os.makedirs(os.path.dirname(os.path.abspath(args.report)), exist_ok=True)
        with open(args.report, "w") as f:
            json.dump({"result": result, "failed": failed,
                       "args": {k: v for k, v in sorted(vars(args).items())}}, f, indent=2)
    for why in failed:
        logger.error(why)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
