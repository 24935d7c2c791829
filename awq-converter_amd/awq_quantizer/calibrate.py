"""python -m awq_quantizer.calibrate — the activation statistics --act_stats reads, from a model
directory and token ids, on the GPU (awq_quantizer/calibration).

  python -m awq_quantizer.calibrate --model_id DIR --output stats.safetensors --input_ids ids.safetensors
  python -m awq_quantizer.calibrate --model_id DIR --output stats.safetensors --text_file corpus.txt \
         --n_samples 128 --seq_len 512

--input_ids: a safetensors file with `input_ids` int64 [n, seq], or a .npy of the same.
--samples_output FILE [--n_sample_tokens 512]: also keeps evenly spread token rows of every linear's
input, written to a second safetensors file (the statistics file is unchanged) for the output-space
loss and report (main --act_samples, verify --act_samples).
--text_file: needs the `tokenizers` package and DIR/tokenizer.json; the text is tokenised,
concatenated and cut into seq_len blocks, the first n_samples kept.
Every argument error exits 1 before any device work.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from typing import List, Optional

from .utils.logger import get_logger


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="awq_quantizer.calibrate", description="Activation statistics for --act_stats")
    p.add_argument("--model_id", type=str, required=True, help="Model directory (config.json + safetensors)")
    p.add_argument("--output", type=str, required=True, help="Statistics file to write (safetensors)")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--input_ids", type=str, help="safetensors with input_ids int64 [n, seq], or a .npy")
    src.add_argument("--text_file", type=str, help="Plain text, tokenised with the model's tokenizer.json")
    p.add_argument("--n_samples", type=int, default=128, help="--text_file: sequences kept")
    p.add_argument("--seq_len", type=int, default=512, help="--text_file: tokens per sequence")
    p.add_argument("--compute_dtype", type=str, default=None, choices=["bfloat16", "float16", "float32"],
                   help="Dtype of the forward (default: the checkpoint's)")
    p.add_argument("--batch_tokens", type=int, default=8192, help="Tokens per micro-batch (whole sequences)")
    p.add_argument("--samples_output", type=str, default=None,
                   help="Also write token samples of every linear's input ('<block>.<group>.samples', a second "
                        "safetensors file) for the output-space loss (--act_samples)")
    p.add_argument("--n_sample_tokens", type=int, default=512, help="--samples_output: token rows kept per input")
    p.add_argument("--device", type=str, default="cuda", help="The GPU to run on (there is no CPU path)")
    p.add_argument("--log_level", type=str, default="INFO", choices=["DEBUG", "INFO", "WARNING", "ERROR", "CRITICAL"])
    return p


def load_ids(args):
    """The token ids of the chosen source (host only)."""
    from .calibration import chunk_text, read_input_ids
    if args.input_ids:
        if not os.path.isfile(args.input_ids):
            raise ValueError(f"--input_ids: {args.input_ids} does not exist")
        return read_input_ids(args.input_ids)
    if args.n_samples <= 0 or args.seq_len <= 0:
        raise ValueError("--n_samples and --seq_len must be positive")
    if not os.path.isfile(args.text_file):
        raise ValueError(f"--text_file: {args.text_file} does not exist")
    tok_path = os.path.join(args.model_id, "tokenizer.json")
    try:
        from tokenizers import Tokenizer
    except ImportError:
        raise ValueError("--text_file needs the `tokenizers` package, which is not installed; tokenise elsewhere "
                         "and pass --input_ids") from None
    if not os.path.isfile(tok_path):
        raise ValueError(f"--text_file needs {tok_path}; tokenise elsewhere and pass --input_ids")
    with open(args.text_file, encoding="utf-8") as f:
        text = f.read()
    return chunk_text(text, Tokenizer.from_file(tok_path), args.seq_len, args.n_samples)


def main(argv: Optional[List[str]] = None) -> int:
    try:
        args = build_parser().parse_args(argv)
    except SystemExit as e:            # argparse exits 2; this tool's argument errors are all 1
        return 0 if e.code in (0, None) else 1
    logger = get_logger(name="awq_calibrate", level=args.log_level)
    try:
        from .calibration import parse_config, read_config
        if args.batch_tokens <= 0:
            raise ValueError("--batch_tokens must be positive")
        if args.samples_output and args.n_sample_tokens <= 0:
            raise ValueError("--n_sample_tokens must be positive")
        if not os.path.isdir(args.model_id):
            raise ValueError(f"--model_id: {args.model_id} is not a directory")
        cfg = read_config(args.model_id)
        ids = load_ids(args)
        parse_config(cfg, seq_len=ids.shape[1], max_id=int(ids.max()))
    except (ValueError, OSError) as e:
        logger.error(str(e))
        return 1
    try:
        from .calibration import calibrate_model, save_act_samples, save_act_stats
        t0 = time.time()
        samples = {} if args.samples_output else None
        stats = calibrate_model(args.model_id, ids, compute_dtype=args.compute_dtype, batch_tokens=args.batch_tokens,
                                device=args.device, logger=logger,
                                n_sample_tokens=args.n_sample_tokens if args.samples_output else 0, samples_out=samples)
        seconds = time.time() - t0
        save_act_stats(stats, args.output)
        if args.samples_output:
            save_act_samples(samples, args.samples_output)
            logger.info(f"Wrote token samples of {len(samples)} inputs to {args.samples_output}")
    except Exception as e:  # noqa: BLE001
        logger.error(f"Calibration failed: {e}")
        return 1
    tokens = int(ids.numel())
    logger.info(f"Wrote activation statistics of {len(stats)} weights to {args.output}")
    logger.info("metrics " + json.dumps({"tokens": tokens, "blocks": int(cfg["num_hidden_layers"]),
                                         "seconds": round(seconds, 4),
                                         "tokens_per_s": round(tokens / max(seconds, 1e-9), 1)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
