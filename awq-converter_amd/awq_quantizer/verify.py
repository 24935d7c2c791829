"""Check a written checkpoint against its source: the quantization-error report of every tensor.

    python -m awq_quantizer.verify --model_id SRC --quantized_dir OUT [--report PATH]
                                   [--device cuda:0] [--worst N]

Reads OUT/metadata.json and the chunk files the CLI wrote (model_chunk_NNNN.pt or .safetensors,
--output_format reference or packed), reads each tensor's original from the safetensors files
under SRC, and computes AWQQuantizer.quantization_error for it: one pass over the weights and the
packed result on the GPU (include/awq_hip.h awq_quant_error).  Logs one line per tensor and the
N worst tensors by snr_db, and writes a JSON report: per-tensor entries and model totals.
Results of --scale_method awq --act_stats carry "input_scale" and quantize W * diag(input_scale):
they are measured against the source scaled the same way (entry "input_scaled": true).
Returns 0, or 1 when the checkpoint cannot be read, a quantized tensor has no source, or the
shapes disagree.  --output_format autoawq directories (model.safetensors in the AutoAWQ GEMM
layout, no metadata.json) are out of scope.
"""
import argparse
import json
import math
import os
import sys
from typing import Callable, Dict, Iterator, List, Optional, Tuple

import torch

from .utils.logger import get_logger

CHUNK_STEM = "model_chunk_{:04d}"          # main.py's layout (reference main.py:485)
_RESULT_KEYS = ("tensor_q", "scales", "zero_points", "qweight", "qzeros", "bits", "group_size", "symmetric",
                "shape", "input_scale")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="awq_quantizer.verify",
                                description="Quantization-error report of a written checkpoint against its source")
    p.add_argument("--model_id", type=str, required=True, help="directory of the source model's safetensors files")
    p.add_argument("--quantized_dir", type=str, required=True,
                   help="output directory of awq_quantizer (--output_format reference or packed)")
    p.add_argument("--report", type=str, default=None,
                   help="JSON report path (default: <quantized_dir>/quantization_error.json)")
    p.add_argument("--device", type=str, default="cuda:0", help="GPU the report is computed on")
    p.add_argument("--worst", type=int, default=5, help="log the N worst tensors by snr_db")
    p.add_argument("--log_level", type=str, default="INFO")
    return p


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


def _split_flat(flat: Dict[str, torch.Tensor]) -> Dict[str, Dict[str, torch.Tensor]]:
    """'<tensor name>.<key>' entries of a safetensors chunk -> nested result dicts."""
    out: Dict[str, Dict[str, torch.Tensor]] = {}
    for full, v in flat.items():
        name, _, key = full.rpartition(".")
        if key not in _RESULT_KEYS or not name:
            raise ValueError(f"unexpected entry {full!r} in a chunk file")
        out.setdefault(name, {})[key] = v
    return out


def iter_results(quantized_dir: str) -> Iterator[Tuple[str, Dict[str, torch.Tensor]]]:
    """(name, result dict) of every tensor of a written checkpoint, chunk by chunk."""
    meta_path = os.path.join(quantized_dir, "metadata.json")
    if not os.path.exists(meta_path):
        hint = ""
        if os.path.exists(os.path.join(quantized_dir, "model.safetensors")) or \
                os.path.exists(os.path.join(quantized_dir, "model.safetensors.index.json")):
            hint = " (this looks like an --output_format autoawq directory, which verify does not read)"
        raise FileNotFoundError(f"{meta_path} is missing{hint}")
    with open(meta_path) as f:
        meta = json.load(f)
    st = meta.get("format") == "safetensors"
    for c in range(int(meta["num_chunks"])):
        path = os.path.join(quantized_dir, CHUNK_STEM.format(c) + (".safetensors" if st else ".pt"))
        if st:
            from safetensors.torch import load_file
            chunk = _split_flat(load_file(path))
        else:
            chunk = torch.load(path, map_location="cpu", weights_only=True)
        for name, res in chunk.items():
            yield name, res


def model_totals(entries: Dict[str, dict]) -> dict:
    """Model totals of per-tensor reports: sums and counts add, the max is the max."""
    from .quantization.awq import error_report
    vals = list(entries.values())
    totals = [math.fsum(e[k] for e in vals) for k in ("sum_abs", "sum_sq", "sum_w_sq")]
    totals.append(max((e["max_abs_error"] for e in vals), default=0.0))
    totals.append(sum(e["nonfinite"] for e in vals))
    out = error_report(sum(e["numel"] for e in vals), totals)
    out["tensors"] = len(vals)
    return out


def write_report(path: str, entries: Dict[str, dict], problems: Dict[str, str], args_echo: dict,
                 skipped: Optional[Dict[str, str]] = None) -> dict:
    """The JSON report: {"tensors": {name: entry}, "totals": ..., "problems": {name: why},
    "skipped": {name: why}} (skipped: small-tensor results, which have no groups to report).
    Non-finite numbers (snr_db of an exact tensor, the mean of an all-non-finite one) are written
    as JSON's Infinity / NaN extensions, which Python's json reads back."""
    report = {"source": args_echo, "tensors": entries, "totals": model_totals(entries), "problems": problems,
              "skipped": skipped or {}}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(report, f, indent=2)
    return report


def worst_tensors(entries: Dict[str, dict], n: int) -> List[str]:
    """The n worst tensors: first those with no finite element at all (nothing of them could be
    measured; their snr_db reads inf because sum_sq is 0), then by ascending snr_db (-inf: an
    all-zero source with an error)."""
    def key(name):
        e = entries[name]
        return (0, 0.0) if e["nonfinite"] >= e["numel"] else (1, e["snr_db"])
    return sorted(entries, key=key)[:max(0, n)]


def verify(args: argparse.Namespace, error_fn: Optional[Callable] = None, logger=None) -> int:
    """error_fn(tensor, result) -> report dict; default: AWQQuantizer.quantization_error on args.device."""
    logger = logger or get_logger(name="awq_verify", level=args.log_level)
    from .model_loading.safetensors_loader import SafetensorsLoader
    try:
        loader = SafetensorsLoader(model_path=args.model_id, logger_level=args.log_level)
        index = {i.name: i for i in loader.tensor_index()}
    except Exception as e:  # noqa: BLE001
        logger.error(f"Failed to read the source model {args.model_id}: {e}")
        return 1
    if error_fn is None:
        from .quantization.awq import AWQQuantizer
        quantizer = AWQQuantizer(device=args.device, logger_name="awq_verify_quantizer", logger_level="WARNING")
        error_fn = quantizer.quantization_error
    entries: Dict[str, dict] = {}
    problems: Dict[str, str] = {}
    skipped: Dict[str, str] = {}
    try:
        for name, res in iter_results(args.quantized_dir):
            info = index.get(name)
            if info is None:
                problems[name] = "no source tensor of this name"
                logger.error(f"{name}: {problems[name]}")
                continue
            shape = tuple(res["shape"].tolist()) if "shape" in res else tuple(res["tensor_q"].shape)
            if tuple(info.shape) != tuple(int(v) for v in shape):
                problems[name] = f"shape {list(shape)} != source shape {list(info.shape)}"
                logger.error(f"{name}: {problems[name]}")
                continue
            try:
                e = error_fn(loader.read(info), res)
            except IndexError as ex:   # a small-tensor result (0-d / 1-d scales): not a group result
                skipped[name] = str(ex)
                logger.warning(f"{name}: skipped ({ex})")
                continue
            except Exception as ex:  # noqa: BLE001
                problems[name] = f"{type(ex).__name__}: {ex}"
                logger.error(f"{name}: {problems[name]}")
                continue
            entries[name] = {k: e[k] for k in ("numel", "nonfinite", "sum_abs", "sum_sq", "sum_w_sq",
                                               "mean_abs_error", "mse", "max_abs_error", "snr_db")}
            # --scale_method awq --act_stats: measured against W * diag(input_scale) (quantization_error)
            entries[name]["input_scaled"] = "input_scale" in res
            logger.info(f"{name}: mean_abs_error {e['mean_abs_error']:.6g}  max {e['max_abs_error']:.6g}  "
                        f"snr {e['snr_db']:.2f} dB  nonfinite {e['nonfinite']}")
    except Exception as e:  # noqa: BLE001
        logger.error(f"Failed to read the quantized checkpoint {args.quantized_dir}: {e}")
        return 1
    finally:
        loader.close()
    for name in worst_tensors(entries, args.worst):
        logger.info(f"worst by snr_db: {name}  {entries[name]['snr_db']:.2f} dB")
    path = args.report or os.path.join(args.quantized_dir, "quantization_error.json")
    report = write_report(path, entries, problems, {"model_id": args.model_id, "quantized_dir": args.quantized_dir},
                          skipped)
    t = report["totals"]
    logger.info(f"{t['tensors']} tensors, {t['numel']} elements: mean_abs_error {t['mean_abs_error']:.6g}  "
                f"snr {t['snr_db']:.2f} dB  nonfinite {t['nonfinite']}; report: {path}")
    return 1 if problems else 0


def main(argv: Optional[List[str]] = None) -> int:
    return verify(parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
