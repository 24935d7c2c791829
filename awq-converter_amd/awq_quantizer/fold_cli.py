"""
The CLI's --fold_scales run: one process, one GPU, the decoder blocks one by one.  main()
imports this module only for such a run.
"""

import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import replace
from typing import Dict, List

import torch

from .model_loading import TensorInfo
from .output import _to_cpu, finish_run, model_type_of, save_autoawq
from .pipeline import TIMINGS, StreamSettings, new_quantizer, quantize_stream_python


def _main_fold_scales(args, cfg: StreamSettings, loader, index: List[TensorInfo], ordered: List[TensorInfo],
                      passthrough: List[TensorInfo], device: str, logger, start: float,
                      act_samples: Dict[str, torch.Tensor] = None) -> int:
    """--fold_scales: the decoder blocks one by one (quantization/block_plan.py) — a block's members
    and producers read together (the next block read ahead on the reader pool), then
    AWQQuantizer.quantize_block, export_autoawq (or export_gptq) per result and D2H; linears in no group
    take the regular path (RTN).  A block that fails is copied unquantized (modules_to_not_convert) with its
    norms and biases left unfolded.  Writes model.safetensors (folded norm weights and biases in
    place of the source's), the configs, and awq_scales.safetensors: every block's "scales".
    act_samples (--search_loss output, --clip_loss output, --rounding gptq): "<block prefix>.<group>.samples"
    -> token samples; each block's four tensors go to quantize_block, with loss="output" and / or
    clip_loss="output"; --rounding gptq sets the quantizer's rounding / gptq_damp and logs every weight's
    output error, round-to-nearest -> compensated."""
    from safetensors.torch import save_file
    from .quantization.act_search import quantize_block
    from .quantization.block_plan import plan_blocks
    by_name = {i.name: i for i in index}
    plan = plan_blocks({i.name: i.shape for i in index}, model_type_of(loader), args.group_size)
    linear = {i.name for i in ordered}
    quantizer = new_quantizer(args, device)
    try:
        quantizer.compute_device()
    except Exception as e:  # noqa: BLE001
        logger.error(f"Quantization on {device} failed: {e}")
        return 1
    gptq = getattr(args, "rounding", "nearest") == "gptq" and act_samples is not None
    if gptq:    # settings of the quantizer, as clip_loss is: quantize_block's signature is pinned
        quantizer.rounding, quantizer.gptq_damp = "gptq", args.gptq_damp
    clip_kw = {"clip": True, **cfg.act_clip} if cfg.act_clip else {}
    output_loss = act_samples is not None and args.search_loss == "output"
    output_clip = act_samples is not None and bool(cfg.act_clip) and args.clip_loss == "output"
    results: Dict[str, Dict[str, torch.Tensor]] = {}
    overrides: Dict[str, torch.Tensor] = {}
    sidecar: Dict[str, torch.Tensor] = {}
    blocks = [b for b in plan if all(m in linear for m in b.members())]
    grouped = {m for b in blocks for m in b.members()}
    rest = [i for i in ordered if i.name not in grouped]
    logger.info(f"Scale folding: {len(blocks)} decoder blocks, {len(grouped)} linears in layer groups, "
                f"{len(rest)} in none (RTN)")
    inside = [i.name for i in rest if any(i.name.startswith(b.prefix + ".") for b in plan)]
    if inside:   # none in llama / mistral / qwen2; one reading a folded norm's output would see x / s unscaled
        logger.warning(f"linears inside a decoder block that belong to no layer group are quantized without an "
                       f"input scale; if one reads a folded norm's output the checkpoint is wrong: {inside}")
    with ThreadPoolExecutor(max_workers=max(1, args.num_workers)) as pool:
        futs = {}

        def submit(k):
            if k < len(blocks) and k not in futs:
                futs[k] = {n: pool.submit(loader.read, by_name[n]) for n in blocks[k].tensor_names()}

        submit(0)
        for k, block in enumerate(blocks):
            submit(k + 1)
            try:
                tensors = {n: f.result() for n, f in futs.pop(k).items()}
                loss_kw = {}
                if output_loss or output_clip or gptq:
                    smp = {g: act_samples[f"{block.prefix}.{g}.samples"] for g in block.groups
                           if f"{block.prefix}.{g}.samples" in act_samples}
                    loss_kw = {"samples": smp, **({"loss": "output"} if output_loss else {})}
                if output_clip:     # (the method's signature has no clip_loss: the function behind it takes it)
                    out = quantize_block(quantizer, tensors, cfg.act_stats, block, **clip_kw, **loss_kw,
                                         clip_loss="output")
                else:
                    out = quantizer.quantize_block(tensors, cfg.act_stats, block, **clip_kw, **loss_kw)
                if cfg.export_gptq:
                    exported = {n: _to_cpu(quantizer.export_gptq(r, cfg.export_gptq))
                                for n, r in out["results"].items()}
                else:
                    exported = {n: _to_cpu(quantizer.export_autoawq(r)) for n, r in out["results"].items()}
                host_folded = _to_cpu(out["folded"])
                host_scales = _to_cpu(out["scales"])
            except Exception as e:  # noqa: BLE001  (the block's linears are copied unquantized)
                logger.error(f"Error quantizing block {block.prefix}: {e}")
                continue
            results.update(exported)
            overrides.update(host_folded)
            sidecar.update(host_scales)
            logger.info(f"Successfully quantized block: {block.prefix} on {device} (folded groups: "
                        f"{[n for n, g in out['groups'].items() if g['folded']]})")
            for gname, g in out["groups"].items():
                if g.get("clip"):
                    logger.info(f"{block.prefix}.{gname}: clip loss {g['clip'].get('loss', 'diag')}, "
                                f"{g['clip']['loss_before']:.6g} -> {g['clip']['loss_after']:.6g}")
                for m, rd in (g.get("rounding") or {}).items():
                    if rd["loss"] is not None:
                        logger.info(f"{m}: gptq rounding, output error {rd['loss_rtn']:.6g} -> {rd['loss']:.6g}"
                                    f"{' (fallback: nearest)' if rd['fallback'] else ''}")
                if g.get("loss"):
                    logger.info(f"{block.prefix}.{gname}: search loss {g['loss']}, winner {g['best']}/"
                                f"{args.search_grid} (diagonal loss: {g['diag_best']}/{args.search_grid})")
    if rest:   # the regular pipeline, RTN: no statistics, no clip search
        quantize_stream_python(replace(cfg, act_stats=None, act_clip=None), loader, rest, quantizer, device,
                               results, threading.Lock(), logger)
    TIMINGS["quantize_s"] = time.time() - start
    quantized = {i.name: results[i.name] for i in ordered if i.name in results}

    def save():
        save_autoawq(quantized, loader, passthrough, args.output_dir, args, logger,
                     failed=[i for i in ordered if i.name not in quantized], overrides=overrides)
        save_file({k: v.contiguous() for k, v in sidecar.items()},
                  os.path.join(args.output_dir, "awq_scales.safetensors"), metadata={"format": "pt"})
    return finish_run(args, ordered, quantized, logger, start, save)
