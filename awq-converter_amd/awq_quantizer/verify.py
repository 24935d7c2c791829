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
shapes disagree.

--output_format autoawq directories (no metadata.json; model.safetensors, or model.safetensors.
index.json and the shards it names, in the AutoAWQ GEMM layout) are read back as well
(verify_autoawq): quant_config.json gives the group size and zero_point; every <layer>.qweight /
.qzeros / .scales triple is imported into the row-major layout (AWQQuantizer.import_autoawq) and
measured against the source's <layer>.weight in the domain it was quantized in, rebuilt from
awq_scales.safetensors when --fold_scales wrote one: first fold_rows(W, <layer>.weight.row_scale),
then input_scale = <layer>.weight.input_scale (quantize_block's order); entries gain "row_folded"
and "layout": "autoawq".  --output_format gptq directories (the same files, with
quantize_config.json saying quant_method "gptq") take the same audit through
AWQQuantizer.import_gptq ("layout": "gptq"); a g_idx that is not k // group_size (act-order is
not supported), a symmetric checkpoint with a stored zero other than 8, and a missing or unknown
checkpoint_format are findings.  With a sidecar the fold itself is audited (fold_audit): one input scale
per layer group, the folded norm weights and producer biases bit for bit.  Every other tensor must
equal the source's bytes (report key "copied").  Any finding is a "problems" entry and makes the
return code 1.  Checkpoints written by AutoAWQ itself are out of scope (parity unpinned).

--act_samples FILE (awq_quantizer.calibrate --samples_output): every linear that has token samples
of its input also gets the output-space figures (quantization_error(samples=): output_sum_sq,
output_ref_sq, output_rel_error, output_snr_db, output_tokens — for a result with input_scale in
the original domain; AutoAWQ layout: against the row-folded source), the totals add the sums, and
a second worst-N list is logged by output_snr_db.  Without the flag the report is unchanged.
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
                   help="output directory of awq_quantizer (--output_format reference, packed or autoawq; "
                        "an autoawq directory written with --fold_scales also has its fold audited)")
    p.add_argument("--report", type=str, default=None,
                   help="JSON report path (default: <quantized_dir>/quantization_error.json)")
    p.add_argument("--device", type=str, default="cuda:0", help="GPU the report is computed on")
    p.add_argument("--worst", type=int, default=5, help="log the N worst tensors by snr_db")
    p.add_argument("--act_samples", type=str, default=None,
                   help="token samples written by awq_quantizer.calibrate --samples_output: every linear that has "
                        "samples also gets the output-space figures (output_sum_sq, output_snr_db, ...)")
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
            hint = " (this looks like an --output_format autoawq directory: verify_autoawq reads those)"
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
    with_output = [e for e in vals if "output_sum_sq" in e]
    if with_output:     # --act_samples: the output-space sums add too
        from .quantization.awq import output_report
        o = output_report(math.fsum(e["output_sum_sq"] for e in with_output),
                          math.fsum(e["output_ref_sq"] for e in with_output), 0)
        del o["output_tokens"]
        out.update(o, output_tensors=len(with_output))
    return out


_OUTPUT_KEYS = ("output_sum_sq", "output_ref_sq", "output_rel_error", "output_snr_db", "output_tokens")


def measure(error_fn: Callable, w: torch.Tensor, res: Dict[str, torch.Tensor], samples: Optional[torch.Tensor]):
    """error_fn's report; with token samples of this linear's input also the output-space figures."""
    return error_fn(w, res) if samples is None else error_fn(w, res, samples=samples)


def output_entry(e: dict) -> dict:
    return {k: e[k] for k in _OUTPUT_KEYS if k in e}


def log_worst(entries: Dict[str, dict], n: int, logger) -> None:
    for name in worst_tensors(entries, n):
        logger.info(f"worst by snr_db: {name}  {entries[name]['snr_db']:.2f} dB")
    for name in worst_by_output(entries, n):
        logger.info(f"worst by output_snr_db: {name}  {entries[name]['output_snr_db']:.2f} dB")


def worst_by_output(entries: Dict[str, dict], n: int) -> List[str]:
    """The n worst tensors by ascending output_snr_db among those measured on samples (NaN first)."""
    have = [k for k, e in entries.items() if "output_snr_db" in e]
    return sorted(have, key=lambda k: (0, 0.0) if entries[k]["output_snr_db"] != entries[k]["output_snr_db"]
                  else (1, entries[k]["output_snr_db"]))[:max(0, n)]


def read_samples(args, logger) -> Optional[Dict[str, torch.Tensor]]:
    """--act_samples: weight name -> samples ({} without the flag); None after logging why not."""
    path = getattr(args, "act_samples", None)
    if not path:
        return {}
    try:
        from .calibration import load_act_samples
        out = load_act_samples(path)
    except Exception as e:  # noqa: BLE001
        logger.error(f"--act_samples: cannot read {path}: {e}")
        return None
    logger.info(f"Loaded token samples for {len(out)} weights from {path}")
    return out


def write_report(path: str, entries: Dict[str, dict], problems: Dict[str, str], args_echo: dict,
                 skipped: Optional[Dict[str, str]] = None, extra: Optional[dict] = None) -> dict:
    """The JSON report: {"tensors": {name: entry}, "totals": ..., "problems": {name: why},
    "skipped": {name: why}} (skipped: small-tensor results, which have no groups to report).
    Non-finite numbers (snr_db of an exact tensor, the mean of an all-non-finite one) are written
    as JSON's Infinity / NaN extensions, which Python's json reads back."""
    report = {"source": args_echo, "tensors": entries, "totals": model_totals(entries), "problems": problems,
              "skipped": skipped or {}}
    report.update(extra or {})     # AutoAWQ directories: "layout", "copied", "fold_audited"
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


def verify(args: argparse.Namespace, error_fn: Optional[Callable] = None, logger=None,
           import_fn: Optional[Callable] = None, fold_fn: Optional[Callable] = None) -> int:
    """error_fn(tensor, result) -> report dict; default: AWQQuantizer.quantization_error on args.device.
    AutoAWQ directories also use import_fn(gemm, group_size, symmetric) (default:
    AWQQuantizer.import_autoawq) and fold_fn(w, s) (default: awq_fold_rows on args.device)."""
    logger = logger or get_logger(name="awq_verify", level=args.log_level)
    samples = read_samples(args, logger)
    if samples is None:
        return 1
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
    if is_autoawq_dir(args.quantized_dir):
        made = []

        def q():    # built on first use: a caller that injects all three functions needs no quantizer
            if not made:
                from .quantization.awq import AWQQuantizer
                made.append(AWQQuantizer(device=args.device, logger_name="awq_verify_import", logger_level="WARNING"))
            return made[0]

        def device_fold(w, s):
            from . import _hip
            dev = q().compute_device()
            return _hip.fold_rows(w.to(dev).contiguous(), s.to(dev, torch.float32).contiguous())

        if is_gptq_dir(args.quantized_dir):     # import_fn also takes the checkpoint_format
            return verify_autoawq(args, loader, index, error_fn,
                                  import_fn or (lambda g, gs, sym, fmt: q().import_gptq(g, gs, sym, fmt)),
                                  fold_fn or device_fold, logger, samples, layout="gptq")
        return verify_autoawq(args, loader, index, error_fn,
                              import_fn or (lambda gemm, gs, sym: q().import_autoawq(gemm, gs, sym)),
                              fold_fn or device_fold, logger, samples)
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
                e = measure(error_fn, loader.read(info), res, samples.get(name))
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
            entries[name].update(output_entry(e))
            logger.info(f"{name}: mean_abs_error {e['mean_abs_error']:.6g}  max {e['max_abs_error']:.6g}  "
                        f"snr {e['snr_db']:.2f} dB  nonfinite {e['nonfinite']}")
    except Exception as e:  # noqa: BLE001
        logger.error(f"Failed to read the quantized checkpoint {args.quantized_dir}: {e}")
        return 1
    finally:
        loader.close()
    log_worst(entries, args.worst, logger)
    path = args.report or os.path.join(args.quantized_dir, "quantization_error.json")
    report = write_report(path, entries, problems, {"model_id": args.model_id, "quantized_dir": args.quantized_dir},
                          skipped)
    t = report["totals"]
    logger.info(f"{t['tensors']} tensors, {t['numel']} elements: mean_abs_error {t['mean_abs_error']:.6g}  "
                f"snr {t['snr_db']:.2f} dB  nonfinite {t['nonfinite']}; report: {path}")
    return 1 if problems else 0


# ---------------------------------------------------------------- AutoAWQ directories
_GEMM_KEYS = ("qweight", "qzeros", "scales")
_ENTRY_KEYS = ("numel", "nonfinite", "sum_abs", "sum_sq", "sum_w_sq", "mean_abs_error", "mse", "max_abs_error",
               "snr_db")


def is_autoawq_dir(quantized_dir: str) -> bool:
    """No metadata.json, and model.safetensors or its sharded index: an --output_format autoawq directory."""
    if os.path.exists(os.path.join(quantized_dir, "metadata.json")):
        return False
    return any(os.path.exists(os.path.join(quantized_dir, f))
               for f in ("model.safetensors", "model.safetensors.index.json"))


def autoawq_files(quantized_dir: str) -> List[str]:
    """model.safetensors, or the shards model.safetensors.index.json names (in name order)."""
    one = os.path.join(quantized_dir, "model.safetensors")
    if os.path.exists(one):
        return [one]
    with open(os.path.join(quantized_dir, "model.safetensors.index.json")) as f:
        wmap = json.load(f)["weight_map"]
    return [os.path.join(quantized_dir, f) for f in sorted(set(wmap.values()))]


def read_quant_config(quantized_dir: str) -> Tuple[dict, Dict[str, str]]:
    """({"group_size", "symmetric", "not_converted"}, problems) of quant_config.json."""
    path = os.path.join(quantized_dir, "quant_config.json")
    problems: Dict[str, str] = {}
    try:
        with open(path) as f:
            cfg = json.load(f)
    except (OSError, ValueError) as e:
        return {}, {"quant_config.json": f"cannot be read: {e}"}
    if cfg.get("w_bit") != 4:
        problems["quant_config.json"] = f"w_bit {cfg.get('w_bit')!r}: only 4-bit AutoAWQ checkpoints are read"
    gs = cfg.get("q_group_size")
    if not isinstance(gs, int) or isinstance(gs, bool) or gs <= 0:
        problems["quant_config.json"] = f"q_group_size {gs!r} is not a positive integer"
    out = {"group_size": gs, "symmetric": not bool(cfg.get("zero_point", True)),
           "not_converted": list(cfg.get("modules_to_not_convert") or [])}
    return out, problems


# ---------------------------------------------------------------- GPTQ directories
GPTQ_FORMATS = ("gptq", "gptq_v2")


def _gptq_settings(quantized_dir: str) -> Optional[dict]:
    """quantize_config.json, else config.json's quantization_config, when it says quant_method
    "gptq"; None otherwise."""
    for fname, key in (("quantize_config.json", None), ("config.json", "quantization_config")):
        try:
            with open(os.path.join(quantized_dir, fname)) as f:
                cfg = json.load(f)
        except (OSError, ValueError):
            continue
        cfg = cfg.get(key) if key else cfg
        if isinstance(cfg, dict) and cfg.get("quant_method") == "gptq":
            return cfg
    return None


def is_gptq_dir(quantized_dir: str) -> bool:
    """An --output_format gptq directory: the files of an autoawq one, and settings that say
    quant_method "gptq"."""
    return is_autoawq_dir(quantized_dir) and _gptq_settings(quantized_dir) is not None


def read_gptq_config(quantized_dir: str) -> Tuple[dict, Dict[str, str]]:
    """({"group_size", "symmetric", "checkpoint_format", "not_converted"}, problems) of a GPTQ
    directory's settings."""
    cfg = _gptq_settings(quantized_dir)
    if cfg is None:
        return {}, {"quantize_config.json": "cannot be read, or its quant_method is not 'gptq'"}
    problems: Dict[str, str] = {}
    if cfg.get("bits") != 4:
        problems["quantize_config.json"] = f"bits {cfg.get('bits')!r}: only 4-bit GPTQ checkpoints are read"
    gs = cfg.get("group_size")
    if not isinstance(gs, int) or isinstance(gs, bool) or gs <= 0:
        problems["quantize_config.json"] = f"group_size {gs!r} is not a positive integer"
    if cfg.get("desc_act"):
        problems["quantize_config.json"] = "desc_act is true: act-order checkpoints are not supported"
    fmt = cfg.get("checkpoint_format")
    if fmt not in GPTQ_FORMATS:
        problems["quantize_config.json"] = (f"checkpoint_format {fmt!r} is missing or unknown (known: "
                                            f"{', '.join(GPTQ_FORMATS)}): the stored zero points cannot be read")
    out = {"group_size": gs, "symmetric": bool(cfg.get("sym", False)), "checkpoint_format": fmt,
           "not_converted": list(cfg.get("modules_to_not_convert") or [])}
    return out, problems


def gptq_findings(gptq: Dict[str, torch.Tensor], group_size: int, symmetric: bool, checkpoint_format: str) -> List[str]:
    """What verify reports of one GPTQ linear before it is imported: a g_idx that is not
    k // group_size, and, symmetric, a stored zero point other than 8."""
    out = []
    g = gptq.get("g_idx")
    K = int(gptq["qweight"].shape[0]) * 8
    if g is None:
        out.append("no g_idx")
    else:
        g = g.to(torch.int64).reshape(-1)
        if g.numel() != K:
            out.append(f"g_idx has {g.numel()} entries for in_features {K}")
        else:
            bad = (g != torch.arange(K, dtype=torch.int64) // group_size).nonzero().reshape(-1)
            if bad.numel():
                k = int(bad[0])
                out.append(f"g_idx[{k}] = {int(g[k])}, not {k // group_size} = k // group_size at {bad.numel()} "
                           f"position(s): act-order (desc_act) checkpoints are not supported")
    if symmetric:
        stored = (8 - (1 if checkpoint_format == "gptq" else 0)) * 0x11111111
        stored -= (1 << 32) if stored >= (1 << 31) else 0
        bad = int((gptq["qzeros"].to(torch.int32) != stored).sum())
        if bad:
            out.append(f"symmetric checkpoint with a stored zero point other than 8 in {bad} qzeros word(s)")
    return out


def same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal dtype, shape and bytes (so NaN payloads and signed zeros count)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def fold_audit(shapes: Dict[str, Tuple[int, ...]], model_type: Optional[str], group_size: int,
               sidecar: Dict[str, torch.Tensor], read_source: Callable[[str], torch.Tensor],
               read_checkpoint: Callable[[str], Optional[torch.Tensor]], fold_fn: Callable) -> Dict[str, str]:
    """Is the fold the checkpoint holds the one its sidecar records?  Per layer group of
    plan_blocks(shapes of the source, model_type) (quantization/block_plan.py):
      * its members carry one identical input_scale in the sidecar (all of them, or none);
      * a "vector" group (attn_in / mlp_in) with a scale s_in: the checkpoint's norm weight equals
        fold_fn(source norm, s_in) bit for bit (a group quantize_block did not fold records ones,
        and x / 1 is x: its norm must be the source's);
      * a "rows" group (attn_out / mlp_out) whose producer has a row_scale in the sidecar: that
        row_scale is the members' input_scale, and the producer's bias, if any, equals
        fold_fn(source bias, row_scale); without a row_scale the bias must be the source's;
      * a group with no sidecar scale: norm and bias equal the source's.
    read_checkpoint(name) returns None for a tensor the checkpoint lacks.  fold_fn(w, s) is
    fold_rows (the GPU's awq_fold_rows in verify; any bit-equal restatement elsewhere).  Returns
    name -> finding, each naming the tensor and the group; plan_blocks refusing the model type is
    one finding."""
    from .quantization.block_plan import plan_blocks
    problems: Dict[str, str] = {}
    try:
        plan = plan_blocks(shapes, model_type, group_size)
    except ValueError as e:
        return {"awq_scales.safetensors": f"fold audit impossible: {e}"}

    def expect(name: str, want: torch.Tensor, where: str, what: str) -> None:
        got = read_checkpoint(name)
        if got is None:
            problems[name] = f"{where}: missing from the checkpoint"
        elif not same_bytes(got, want):
            problems[name] = f"{where}: {what}"

    for block in plan:
        for g in block.groups.values():
            where = f"group {block.prefix}:{g.name}"
            have = [m for m in g.members if f"{m}.input_scale" in sidecar]
            s = sidecar[f"{have[0]}.input_scale"] if have else None
            for m in g.members:
                if have and m not in have:
                    problems[f"{m}.input_scale"] = f"{where}: no input_scale while {have[0]} has one"
                elif have and not same_bytes(sidecar[f"{m}.input_scale"], s):
                    problems[f"{m}.input_scale"] = f"{where}: differs from {have[0]}'s input_scale (one input, one scale)"
            if not g.producers:
                continue
            if g.fold == "vector":
                norm = g.producers[0]
                src = read_source(norm)
                if s is not None:
                    expect(norm, fold_fn(src, s), where, "is not fold_rows(source norm weight, input_scale)")
                else:
                    expect(norm, src, where, "differs from the source's although the group has no scale")
            else:
                pw = g.producers[0]
                rs = sidecar.get(f"{pw}.row_scale")
                if rs is not None and s is not None and not same_bytes(rs, s):
                    problems[f"{pw}.row_scale"] = f"{where}: differs from the input_scale of {g.members[0]}"
                elif rs is not None and s is None:
                    problems[f"{pw}.row_scale"] = f"{where}: a row_scale without the input_scale of {g.members[0]}"
                for pb in g.producers[1:]:
                    src = read_source(pb)
                    if rs is not None:
                        expect(pb, fold_fn(src, rs), where, "is not fold_rows(source bias, row_scale)")
                    else:
                        expect(pb, src, where, "differs from the source's although the producer is not row-folded")
    return problems


def audited_tensors(shapes: Dict[str, Tuple[int, ...]], model_type: Optional[str], group_size: int) -> set:
    """The norm weights and producer biases fold_audit judges (empty when plan_blocks refuses)."""
    from .quantization.block_plan import plan_blocks
    try:
        plan = plan_blocks(shapes, model_type, group_size)
    except ValueError:
        return set()
    return {p for b in plan for g in b.groups.values()
            for p in (g.producers[:1] if g.fold == "vector" else g.producers[1:])}


def verify_autoawq(args: argparse.Namespace, loader, index: Dict[str, object], error_fn: Callable,
                   import_fn: Callable, fold_fn: Callable, logger,
                   samples: Optional[Dict[str, torch.Tensor]] = None, layout: str = "autoawq") -> int:
    """verify() for an --output_format autoawq directory (see the module docstring).
    import_fn(gemm, group_size, symmetric) -> quantize_packed()-shaped dict; fold_fn(w, s) = fold_rows.
    layout "gptq": an --output_format gptq directory, the same audit; import_fn then also takes
    the checkpoint_format, and gptq_findings() are problems of their linear."""
    from safetensors import safe_open
    d = args.quantized_dir
    entries: Dict[str, dict] = {}
    skipped: Dict[str, str] = {}
    copied: List[str] = []
    gptq = layout == "gptq"
    cfg, problems = read_gptq_config(d) if gptq else read_quant_config(d)

    def problem(name: str, why: str) -> None:
        problems[name] = why
        logger.error(f"{name}: {why}")

    path = args.report or os.path.join(d, "quantization_error.json")
    echo = {"model_id": args.model_id, "quantized_dir": d}
    if problems:    # without the settings nothing below can be judged
        for name, why in problems.items():
            logger.error(f"{name}: {why}")
        loader.close()
        write_report(path, entries, problems, echo, skipped, extra={"layout": layout, "copied": copied,
                                                                    "fold_audited": False})
        return 1
    handles = []
    try:
        where: Dict[str, object] = {}
        for shard in autoawq_files(d):
            h = safe_open(shard, framework="pt")
            handles.append(h)
            for k in h.keys():
                where[k] = h
        sidecar: Dict[str, torch.Tensor] = {}
        side_path = os.path.join(d, "awq_scales.safetensors")
        has_sidecar = os.path.exists(side_path)
        if has_sidecar:
            from safetensors.torch import load_file
            sidecar = load_file(side_path)
        read_ckpt = lambda n: where[n].get_tensor(n) if n in where else None
        layers = sorted({n.rpartition(".")[0] for n in where if n.rpartition(".")[2] in _GEMM_KEYS
                         and all(f"{n.rpartition('.')[0]}.{k}" in where for k in _GEMM_KEYS)})
        in_triple = {f"{l}.{k}" for l in layers for k in _GEMM_KEYS + (("g_idx",) if gptq else ())}
        for layer in layers:
            name = f"{layer}.weight"
            info = index.get(name)
            if info is None:
                problem(name, "no source tensor of this name")
                continue
            if layer in cfg["not_converted"]:
                problem(name, "quantized although quant_config.json lists it in modules_to_not_convert")
                continue
            gemm = {k: read_ckpt(f"{layer}.{k}") for k in _GEMM_KEYS}
            if gemm["qweight"].dim() != 2:
                shape = tuple(gemm["qweight"].shape)
            elif gptq:
                shape = (int(gemm["qweight"].shape[1]), int(gemm["qweight"].shape[0]) * 8)
            else:
                shape = (int(gemm["qweight"].shape[1]) * 8, int(gemm["qweight"].shape[0]))
            if tuple(info.shape) != shape:
                problem(name, f"shape {list(shape)} != source shape {list(info.shape)}")
                continue
            try:
                if gptq:
                    gemm["g_idx"] = read_ckpt(f"{layer}.g_idx")
                    found = gptq_findings(gemm, cfg["group_size"], cfg["symmetric"], cfg["checkpoint_format"])
                    if found:
                        problem(name, "; ".join(found))
                        continue
                    res = import_fn(gemm, cfg["group_size"], cfg["symmetric"], cfg["checkpoint_format"])
                else:
                    res = import_fn(gemm, cfg["group_size"], cfg["symmetric"])
                w = loader.read(info)
                row_scale = sidecar.get(f"{name}.row_scale")
                if row_scale is not None:
                    w = fold_fn(w, row_scale)
                in_scale = sidecar.get(f"{name}.input_scale")
                if in_scale is not None:
                    res = dict(res, input_scale=in_scale)
                e = measure(error_fn, w, res, (samples or {}).get(name))
            except Exception as ex:  # noqa: BLE001
                problem(name, f"{type(ex).__name__}: {ex}")
                continue
            entries[name] = {k: e[k] for k in _ENTRY_KEYS}
            entries[name].update(input_scaled=in_scale is not None, row_folded=row_scale is not None,
                                 layout=layout)
            entries[name].update(output_entry(e))
            logger.info(f"{name}: mean_abs_error {e['mean_abs_error']:.6g}  max {e['max_abs_error']:.6g}  "
                        f"snr {e['snr_db']:.2f} dB  nonfinite {e['nonfinite']}")
        judged = set()
        if has_sidecar:
            from .output import model_type_of
            shapes = {n: tuple(i.shape) for n, i in index.items()}
            for name, why in fold_audit(shapes, model_type_of(loader), cfg["group_size"], sidecar,
                                        lambda n: loader.read(index[n]), read_ckpt, fold_fn).items():
                problem(name, why)
            judged = audited_tensors(shapes, model_type_of(loader), cfg["group_size"])
            for k in sidecar:   # every sidecar scale belongs to a quantized linear of the checkpoint
                lname = k.rpartition(".")[0]
                if lname not in entries and lname not in problems and k not in problems:
                    problem(k, "sidecar scale of a tensor that is not a quantized linear of the checkpoint")
        # every other tensor: the source's bytes (the audit has judged the folded norms and biases)
        for name in sorted(n for n in where if n not in in_triple):
            info = index.get(name)
            if info is None:
                problem(name, "copied tensor with no source tensor of this name")
                continue
            copied.append(name)
            if name in judged:
                continue
            if not same_bytes(read_ckpt(name), loader.read(info)):
                problem(name, "copied tensor differs from the source's bytes")
        quantized_src = {f"{l}.weight" for l in layers}
        for name in index:
            if name not in where and name not in quantized_src:
                problem(name, "source tensor missing from the checkpoint")
    except Exception as e:  # noqa: BLE001
        logger.error(f"Failed to read the quantized checkpoint {d}: {e}")
        return 1
    finally:
        loader.close()
        del handles
    log_worst(entries, args.worst, logger)
    report = write_report(path, entries, problems, echo, skipped,
                          extra={"layout": layout, "copied": copied, "fold_audited": has_sidecar})
    t = report["totals"]
    logger.info(f"{t['tensors']} tensors, {t['numel']} elements: mean_abs_error {t['mean_abs_error']:.6g}  "
                f"snr {t['snr_db']:.2f} dB  nonfinite {t['nonfinite']}; {len(copied)} copied; report: {path}")
    return 1 if problems else 0


def main(argv: Optional[List[str]] = None) -> int:
    return verify(parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
