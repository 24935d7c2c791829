"""
The CLI's flags (reference main.py:22-159 plus this project's additions) and the rules on how
they combine.  check_flags / check_args are pure: main() logs what they return and exits 1.
"""

import argparse
from typing import Dict, List, Optional

import torch


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="AWQ Quantizer CLI")
    p.add_argument("--model_id", type=str, required=True, help="Model ID on HuggingFace Hub or path to local model")
    p.add_argument("--output_dir", type=str, required=True, help="Directory to save quantized model")
    p.add_argument("--bits", type=int, default=4, choices=[4, 8], help="Number of bits for quantization")
    p.add_argument("--group_size", type=int, default=128, help="Group size for quantization")
    p.add_argument("--symmetric", action="store_true", help="Use symmetric quantization")
    p.add_argument("--zero_point", type=str, default="minmax", choices=["none", "minmax", "percentile"],
                   help="Zero point calibration method")
    p.add_argument("--percentile", type=float, default=0.99, help="Percentile for zero point calibration")
    p.add_argument("--scale_method", type=str, default="mse", choices=["minmax", "mse", "search", "awq"],
                   help="Scale calibration method (minmax/mse: round-to-nearest as the reference; "
                        "search: per-group clip search, opt-in extension)")
    p.add_argument("--search_grid", type=int, default=20, help="scale_method=search / awq: grid size")
    p.add_argument("--act_stats", type=str, default=None,
                   help="scale_method=awq: safetensors file of per-input-channel activation statistics, "
                        "'<weight name>.x_mean' (mean |x|) and '<weight name>.x_sq' (mean x^2), fp32 [in_features]; "
                        "weights without statistics are quantized RTN")
    p.add_argument("--calib_ids", type=str, default=None,
                   help="scale_method=awq: instead of --act_stats, token ids (safetensors with input_ids int64 "
                        "[n, seq], or a .npy) to calibrate on first: the statistics come from a forward of the model "
                        "on the GPU (awq_quantizer.calibrate; llama / mistral / qwen2)")
    p.add_argument("--no_duo_scaling", action="store_true",
                   help="scale_method=awq: channel scales x_mean^r instead of x_mean^r / w_mean^(1-r)")
    p.add_argument("--search_max_shrink", type=float, default=0.5,
                   help="scale_method=search: largest shrink of the group range tried")
    p.add_argument("--act_clip", action="store_true",
                   help="scale_method=awq with --act_stats: after the channel-scale search, an activation-aware "
                        "clip search per group (packed output only)")
    p.add_argument("--fold_scales", action="store_true",
                   help="scale_method=awq with --act_stats and --output_format autoawq: search one input scale per "
                        "layer group of every decoder block (q/k/v, o, gate/up, down), fold 1/s into the op producing "
                        "that input (norm weight, v_proj / up_proj rows) and write a loadable activation-aware "
                        "AutoAWQ checkpoint plus awq_scales.safetensors (llama / mistral / qwen2 tensor names)")
    p.add_argument("--search_loss", type=str, default="diag", choices=["diag", "output"],
                   help="--fold_scales: how the scale search scores a candidate. diag: the diagonal loss from the "
                        "statistics; output: the layer group's output error on token samples (--act_samples, or "
                        "collected by the --calib_ids forward)")
    p.add_argument("--act_samples", type=str, default=None,
                   help="--search_loss output / --clip_loss output: token samples written by awq_quantizer.calibrate "
                        "--samples_output")
    p.add_argument("--n_sample_tokens", type=int, default=512,
                   help="--search_loss output / --clip_loss output with --calib_ids: token rows kept per linear input")
    p.add_argument("--clip_loss", type=str, default="diag", choices=["diag", "output"],
                   help="--act_clip with --fold_scales: how the clip search scores a shrink. diag: the diagonal loss "
                        "from the statistics; output: the error at the linear's output on token samples "
                        "(--act_samples, or collected by the --calib_ids forward), the published objective")
    p.add_argument("--clip_grid", type=int, default=20, help="--act_clip: grid size of the range shrinks")
    p.add_argument("--clip_max_shrink", type=float, default=0.5,
                   help="--act_clip: largest shrink of the group range tried")
    p.add_argument("--rounding", type=str, default="nearest", choices=["nearest", "gptq"],
                   help="--fold_scales: how the fields are chosen once the scales are. nearest: round to nearest; "
                        "gptq: GPTQ's error-compensated rounding on token samples (--act_samples, or collected by the "
                        "--calib_ids forward) after the scale search; not with --act_clip")
    p.add_argument("--gptq_damp", type=float, default=0.01,
                   help="--rounding gptq: the fraction of the Hessian's mean diagonal added to its diagonal")
    p.add_argument("--per_channel", action="store_true", help="Use per-channel quantization")
    p.add_argument("--device", type=str, default="cuda" if torch.cuda.is_available() else "cpu",
                   help="Device to use for quantization (cuda, cuda:0, cuda:1, cpu, or 'all' for all GPUs)")
    p.add_argument("--num_workers", type=int, default=4,
                   help="Number of host threads reading weights ahead of the GPU (per GPU)")
    p.add_argument("--max_memory", type=float, default=0.8,
                   help="Maximum fraction of GPU memory to use (0.0-1.0)")
    p.add_argument("--multi_gpu", action="store_true", help="Use all available GPUs for processing (overrides --device)")
    p.add_argument("--batch_size", type=int, default=10, help="Number of tensors to process in each batch")
    p.add_argument("--prefetch_factor", type=int, default=2,
                   help="Batches of tensors read ahead of the GPU (higher values use more host memory)")
    p.add_argument("--memory_efficient", action="store_true",
                   help="Enable memory-efficient mode (release cached GPU memory after every batch)")
    p.add_argument("--log_level", type=str, default="INFO", choices=["DEBUG", "INFO", "WARNING", "ERROR", "CRITICAL"],
                   help="Logging level")
    p.add_argument("--log_file", type=str, help="Log file path")
    p.add_argument("--save_safetensors", action="store_true", help="Save in safetensors format instead of pytorch format")
    p.add_argument("--chunk_size", type=int, default=10, help="Number of tensors to save in each chunk (for large models)")
    # extension (not in the reference)
    p.add_argument("--output_format", type=str, default="reference", choices=["reference", "packed", "autoawq", "gptq"],
                   help="reference: int32 tensor_q/zero_points + fp16 scales per tensor (reference layout); "
                        "packed: int32 qweight/qzeros (bits-packed) + fp16 scales; "
                        "autoawq: a 4-bit checkpoint in AutoAWQ's GEMM layout (linear weights quantized, "
                        "everything else copied) + quant_config.json; "
                        "gptq: the same in AutoGPTQ's 4-bit layout (desc_act false; --symmetric is honoured) + "
                        "quantize_config.json")
    p.add_argument("--gptq_format", type=str, default="gptq", choices=["gptq", "gptq_v2"],
                   help="--output_format gptq: the checkpoint_format. gptq (v1, what transformers and vLLM read) "
                        "stores zero point - 1 modulo 16; gptq_v2 stores the zero point itself")
    p.add_argument("--dist_output", type=str, default="per_rank", choices=["per_rank", "gather"],
                   help="torchrun mode: per_rank = every rank writes its own chunk files (rank 0 adds "
                        "metadata.json over all of them); gather = results sent to rank 0, which writes everything")
    p.add_argument("--stream_engine", type=str, default="native", choices=["native", "python"],
                   help="native: the C++ read -> H2D -> quantize -> D2H pipeline of libawq_hip.so (awq_stream_*); "
                        "python: the same pipeline driven from Python (the round-2 path; also used for "
                        "--act_stats and --output_format autoawq)")
    return p


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    """Command-line arguments (reference main.py:22-159)."""
    return build_parser().parse_args(argv)


def wants_samples(args) -> bool:
    """A search of this run scores its candidates on token samples, or --rounding gptq solves on them."""
    return args.search_loss == "output" or args.clip_loss == "output" or getattr(args, "rounding", "nearest") == "gptq"


def has_stats(args) -> bool:
    """Activation statistics come with this run, from a file or from a calibration forward."""
    return bool(args.act_stats or args.calib_ids)


def act_clip_of(args) -> Optional[Dict[str, float]]:
    """--act_clip's search settings, as the pipeline and quantize_block take them."""
    return {"clip_grid": args.clip_grid, "clip_max_shrink": args.clip_max_shrink} if args.act_clip else None


AUTOAWQ_NEEDS_4_BITS = "--output_format autoawq writes 4-bit checkpoints (AutoAWQ GEMM layout)"
GPTQ_NEEDS_4_BITS = "--output_format gptq writes 4-bit checkpoints (AutoGPTQ layout, desc_act false)"
GPTQ_ONE_PROCESS = "--output_format gptq runs in one process (it is not written under torchrun)"
# the formats that write a loadable checkpoint: linear weights quantized, everything else copied
CHECKPOINT_FORMATS = ("autoawq", "gptq")


def check_flags(args) -> Optional[str]:
    """The rules that need nothing but the flags: main() applies them before it touches a
    device or the model.  The first error's message, or None."""
    if args.calib_ids and args.act_stats:
        return "--calib_ids and --act_stats are mutually exclusive: the statistics come from one of them"
    if args.fold_scales and (args.scale_method != "awq" or not has_stats(args)
                             or args.output_format not in CHECKPOINT_FORMATS):
        return "--fold_scales needs --scale_method awq, --act_stats and --output_format autoawq"
    if args.search_loss == "output":
        if not args.fold_scales:
            return "--search_loss output needs --fold_scales (and so --scale_method awq and --output_format autoawq)"
        if args.act_samples and args.calib_ids:
            return "--act_samples and --calib_ids both give token samples: the samples come from one of them"
        if not args.act_samples and not args.calib_ids:
            return ("--search_loss output needs token samples: --act_samples FILE (awq_quantizer.calibrate "
                    "--samples_output), or --calib_ids")
        if args.calib_ids and args.n_sample_tokens <= 0:
            return "--n_sample_tokens must be positive"
    if args.clip_loss == "output":
        if not args.act_clip:
            return "--clip_loss output needs --act_clip"
        if not args.fold_scales:
            return "--clip_loss output needs --fold_scales (and so --scale_method awq and --output_format autoawq)"
        if args.act_samples and args.calib_ids:
            return "--act_samples and --calib_ids both give token samples: the samples come from one of them"
        if not args.act_samples and not args.calib_ids:
            return ("--clip_loss output needs token samples: --act_samples FILE (awq_quantizer.calibrate "
                    "--samples_output), or --calib_ids")
        if args.calib_ids and args.n_sample_tokens <= 0:
            return "--n_sample_tokens must be positive"
    if args.act_samples and not wants_samples(args):
        return "--act_samples is read by --search_loss output"
    if getattr(args, "rounding", "nearest") == "gptq":
        if not args.fold_scales:
            return "--rounding gptq needs --fold_scales (and so --scale_method awq and a checkpoint --output_format)"
        if args.act_samples and args.calib_ids:
            return "--act_samples and --calib_ids both give token samples: the samples come from one of them"
        if not args.act_samples and not args.calib_ids:
            return ("--rounding gptq needs token samples: --act_samples FILE (awq_quantizer.calibrate "
                    "--samples_output), or --calib_ids")
        if args.calib_ids and args.n_sample_tokens <= 0:
            return "--n_sample_tokens must be positive"
        if args.act_clip:
            return "--rounding gptq refuses --act_clip: the solver moves the ranges the clip search chose"
        if not 0.0 < getattr(args, "gptq_damp", 0.01) < 1.0:
            return "--gptq_damp must be in (0, 1)"
    return None


def check_args(args, world: int, n_devices: int, model_type: Optional[str]) -> Optional[str]:
    """Every rule on how the flags combine, in the order main() reports them: the first error's
    message, or None for a run that may start.  world: torchrun's WORLD_SIZE (1 without it);
    n_devices: GPUs this process drives; model_type: config.json's, if any (only --fold_scales
    asks)."""
    err = check_flags(args)
    if err:
        return err
    stats = has_stats(args)
    autoawq = args.output_format == "autoawq"
    gptq = args.output_format == "gptq"
    if autoawq and args.bits != 4:
        return AUTOAWQ_NEEDS_4_BITS
    if gptq and args.bits != 4:
        return GPTQ_NEEDS_4_BITS
    if gptq and world > 1:
        return GPTQ_ONE_PROCESS
    if args.fold_scales:
        from .quantization.block_plan import SUPPORTED
        if model_type not in SUPPORTED:
            return (f"--fold_scales knows the block layout of model types {', '.join(SUPPORTED)}; "
                    f"config.json says {model_type!r}")
        if world > 1:
            return "--fold_scales runs in one process (sharding by block under torchrun is not implemented)"
        if n_devices > 1:
            return (f"--fold_scales runs on one GPU, not on {n_devices} (--multi_gpu / --device all): "
                    f"name one with --device")
    if args.act_clip:
        if args.scale_method != "awq" or not stats:
            return "--act_clip needs --scale_method awq and --act_stats"
        if args.output_format != "packed" and not args.fold_scales:
            return "--act_clip writes packed results only: use --output_format packed"
        if args.clip_grid < 1 or not 0.0 <= args.clip_max_shrink <= 1.0:
            return "--act_clip needs --clip_grid >= 1 and --clip_max_shrink in [0, 1]"
    if stats:
        if args.scale_method != "awq":
            return f"{'--calib_ids' if args.calib_ids else '--act_stats'} needs --scale_method awq"
        if gptq and not args.fold_scales:
            return ("--act_stats with --output_format gptq: the searched input scales must be folded "
                    "into the ops producing each input first; use --output_format packed or reference "
                    "(results carry 'input_scale'), or add --fold_scales")
        if autoawq and not args.fold_scales:
            return ("--act_stats with --output_format autoawq: the searched input scales must be folded "
                    "into the ops producing each input first; use --output_format packed or reference "
                    "(results carry 'input_scale'), or add --fold_scales")
    return None
