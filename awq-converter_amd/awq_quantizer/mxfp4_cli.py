"""--output_format mxfp4: every linear weight the checkpoint formats convert, with
in_features % 32 == 0, as OCP microscaling FP4; every other tensor copied.  One process, one device,
tensor by tensor through AWQQuantizer.quantize_mxfp4 (the native streaming pipeline does not know the
format).  The directory: model.safetensors with `<prefix>.weight` (uint8 [N, K / 2]) and
`<prefix>.weight_scale` (uint8 [N, K / 32]) per converted linear, and config.json with a
`quantization_config` (output.write_mxfp4_config).

--mxfp4_rounding gptq: a linear whose layer group (block_plan.plan_blocks) has token
samples `<block prefix>.<group>.samples` in --act_samples goes through quantize_gptq_mxfp4; the Hessian
and its factor are built once per group and every member is solved against them.  A linear without
samples (lm_head, ungrouped, a model type block_plan does not know) rounds to nearest.

--mxfp4_act_scales --act_stats FILE: the decoder blocks of plan_blocks(..., 32) one by one
through AWQQuantizer.quantize_block_mxfp4; the folded norm weights and biases are written in place of the
source's, awq_scales.safetensors holds every block's scales (the keys --fold_scales writes) and the
quantization_config records "input_scales": "awq".  A linear in no block, or of a block that failed, is
quantized as without the flag."""
import time
from typing import Dict, List, Optional

from .model_loading import TensorInfo
from .output import TIMINGS, finish_run, model_type_of, save_mxfp4
from .quantization.linear_weights import CONV1D_MODEL_TYPES, is_linear_weight
from .quantization.mxfp4 import BLOCK


def sample_keys(index: List[TensorInfo], linear: List[TensorInfo], mtype: Optional[str]) -> Dict[str, str]:
    """linear weight name -> the key of its layer group's samples, for the linears plan_blocks groups."""
    from .quantization.block_plan import SUPPORTED, plan_blocks
    if mtype not in SUPPORTED:
        return {}
    names = {i.name for i in linear}
    plan = plan_blocks({i.name: tuple(i.shape) for i in index}, mtype, BLOCK)
    return {m: f"{b.prefix}.{g.name}.samples" for b in plan for g in b.groups.values() for m in g.members if m in names}


def main_mxfp4(args, loader, index: List[TensorInfo], ordered: List[TensorInfo], device: str, logger,
               start: float, act_samples: Optional[dict] = None, act_stats: Optional[dict] = None) -> int:
    import torch

    from .quantization.awq import AWQQuantizer
    mtype = model_type_of(loader)
    if mtype in CONV1D_MODEL_TYPES:
        logger.warning(f"model_type {mtype}: Conv1D projection weights ([in, out]) are copied unquantized")
    linear = [i for i in ordered if is_linear_weight(i, BLOCK, mtype)]
    names = {i.name for i in linear}
    passthrough = [i for i in index if i.name not in names]
    rule = args.mxfp4_scale or "floor"
    gptq = getattr(args, "mxfp4_rounding", None) == "gptq"
    logger.info(f"MXFP4 export (scale rule {rule}, rounding {'gptq' if gptq else 'nearest'}): {len(linear)} linear "
                f"weights quantized, {len(passthrough)} copied")
    q = AWQQuantizer(device=device, logger_name="awq_mxfp4_quantizer", logger_level=args.log_level)
    keys, factors, n_nearest, n_fallback = {}, {}, 0, 0
    if gptq:
        from .quantization import gptq_mxfp4 as gm
        q.gptq_factor = args.gptq_factor
        keys = sample_keys(index, linear, mtype)
    quantized, failed = {}, []
    overrides, sidecar = {}, {}
    if act_stats is not None:
        from .quantization.block_plan import plan_blocks
        by_name = {i.name: i for i in index}
        plan = plan_blocks({i.name: tuple(i.shape) for i in index}, mtype, BLOCK)
        blocks = [b for b in plan if all(m in names for m in b.members())]
        logger.info(f"--mxfp4_act_scales: {len(blocks)} decoder blocks, {sum(len(b.members()) for b in blocks)} linears "
                    f"in layer groups")
        for block in blocks:
            try:
                out = q.quantize_block_mxfp4({n: loader.read(by_name[n]) for n in block.tensor_names()}, act_stats,
                                             block, scale_rule=rule)
                done = {n: {"codes": r["codes"].cpu(), "scales": r["scales"].cpu()} for n, r in out["results"].items()}
                host_folded = {n: t.cpu() for n, t in out["folded"].items()}
                host_scales = {n: t.cpu() for n, t in out["scales"].items()}
            except Exception as e:  # noqa: BLE001  (the block's linears take the plain path below, nothing folded)
                logger.error(f"Error quantizing block {block.prefix}: {e}")
                continue
            quantized.update(done)
            overrides.update(host_folded)
            sidecar.update(host_scales)
            logger.info(f"Successfully quantized block: {block.prefix} (folded groups: "
                        f"{[n for n, g in out['groups'].items() if g['folded']]})")
    for info in linear:
        if info.name in quantized:
            continue
        try:
            w = loader.read(info)
            xs = (act_samples or {}).get(keys.get(info.name))
            if gptq and xs is not None and xs.dim() == 2 and xs.shape[1] == w.shape[1]:
                key = keys[info.name]
                if key not in factors:      # once per layer group: q / k / v share one, gate / up share one
                    x32 = xs.to(q.compute_device()).float()
                    H = x32.t() @ x32
                    factors[key] = gm.prepare(H, args.gptq_damp, args.gptq_factor) if bool(torch.isfinite(H).all()) else None
                r = q.quantize_mxfp4(w, rule) if factors[key] is None else \
                    gm.quantize_gptq_mxfp4(q, w, xs, scale_rule=rule, damp=args.gptq_damp, factor=factors[key])
                n_fallback += int(factors[key] is None or r["rounding"]["fallback"])
            else:
                n_nearest += int(gptq)
                r = q.quantize_mxfp4(w, rule)
            quantized[info.name] = {"codes": r["codes"].cpu(), "scales": r["scales"].cpu()}
        except Exception as e:  # noqa: BLE001  (skip and copy, like the other checkpoint formats)
            logger.error(f"Error quantizing tensor: {info.name}, error: {e}")
            failed.append(info)
    if gptq:
        logger.info(f"--mxfp4_rounding gptq: {len(quantized) - n_nearest} linear weights solved on their samples "
                    f"({n_fallback} fell back), {n_nearest} without samples rounded to nearest")
    TIMINGS["quantize_s"] = time.time() - start
    rounding = {"rounding": "gptq", "damp": args.gptq_damp} if gptq else {"rounding": "nearest"}
    if act_stats is not None:
        rounding["input_scales"] = "awq"
    quantized = {i.name: quantized[i.name] for i in linear if i.name in quantized}      # the source's order

    def save():
        save_mxfp4(quantized, loader, passthrough, args.output_dir, rule, logger, failed, rounding, overrides)
        if act_stats is not None:
            import os

            from safetensors.torch import save_file
            save_file({k: v.contiguous() for k, v in sidecar.items()},
                      os.path.join(args.output_dir, "awq_scales.safetensors"), metadata={"format": "pt"})
    return finish_run(args, linear, quantized, logger, start, save)
