"""Activation-aware MXFP4: act_search.py's per-input-channel scale search scored on the
MXFP4 grid (include/awq_hip.h awq_act_search_losses_mxfp4), the winner quantized in one pass
(awq_quantize_mxfp4_scaled).  Behind AWQQuantizer.quantize_layer_group_mxfp4 / quantize_block_mxfp4.

The format fixes the block (32 along K) and the element type: of the quantizer only search_grid and
duo_scaling are consulted (w_mean is taken at group size 32).  A power-of-two block scale has no range
to shrink, so there is no clip step, and GPTQ rounding on top of the searched scales is not composed
(quantize_gptq_mxfp4 keeps refusing an input scale).
"""
from typing import Dict, Optional, Tuple

import torch

from .. import _hip
from .act_search import group_inputs, group_stats
from .mxfp4 import BLOCK, FORMAT, SCALE_RULES, check_weight


def _result(codes, scales, N, K, rule) -> dict:
    return {"codes": codes, "scales": scales, "format": FORMAT, "scale_rule": rule,
            "shape": torch.tensor([N, K], dtype=torch.int64)}


def quantize_layer_group_mxfp4(q, weights: Dict[str, torch.Tensor], activations: Optional[torch.Tensor] = None, *,
                               x_mean: Optional[torch.Tensor] = None, x_sq: Optional[torch.Tensor] = None,
                               scale_rule: str = "floor", table: Optional[torch.Tensor] = None) -> dict:
    """The search over one layer group (linears [R_j, K] reading the same input), then every weight as
    MXFP4 of W * diag(input_scale).  -> {"results": {name: a quantize_mxfp4 result + "input_scale"},
    "input_scale" fp32 [K], "best", "ratio", "losses" fp64 [search_grid], "table"}."""
    if scale_rule not in SCALE_RULES:
        raise ValueError(f"scale_rule must be one of {list(SCALE_RULES)}, got {scale_rule!r}")
    for w in weights.values():
        check_weight(w)
    dev = q.compute_device()
    ws, _, x_sq, _, table = group_inputs(weights, dev, group_size=BLOCK, n_grid=q.search_grid,
                                         duo_scaling=q.duo_scaling, activations=activations, x_mean=x_mean,
                                         x_sq=x_sq, table=table)
    part = _hip.act_search_losses_mxfp4(ws, x_sq, table, scale_rule)
    losses, best, s = _hip.act_search_select(part, table)
    results = {}
    for name, w in zip(weights, ws):
        N, K = w.shape
        codes = torch.empty((N, K // 2), dtype=torch.uint8, device=dev)
        scales = torch.empty((N, K // BLOCK), dtype=torch.uint8, device=dev)
        _hip.quantize_mxfp4_scaled(w, s, scale_rule, codes, scales)
        results[name] = dict(_result(codes, scales, N, K, scale_rule), input_scale=s)
    best = int(best.item())
    q.logger.info(f"awq mxfp4 search over {list(weights)}: ratio {best}/{q.search_grid}")
    return {"results": results, "input_scale": s, "best": best, "ratio": best / q.search_grid, "losses": losses,
            "table": table}


def quantize_block_mxfp4(q, tensors: Dict[str, torch.Tensor], stats: Dict[str, Tuple[torch.Tensor, torch.Tensor]],
                         block, *, scale_rule: str = "floor") -> dict:
    """One decoder block in quantize_block's order: the out groups, their row folds (awq_fold_rows), the
    in groups, their norm folds.  A group without statistics, or not foldable, is quantized with
    quantize_mxfp4 and its scale is ones.  -> quantize_block's keys: {"results": name -> a quantize_mxfp4
    result, "folded", "scales", "groups"}."""
    dev = q.compute_device()
    results, folded, scales, report = {}, {}, {}, {}
    current: Dict[str, torch.Tensor] = {}     # device tensors, row-folded producers replaced

    def dev_t(name: str) -> torch.Tensor:
        if name not in current:
            if name not in tensors:
                raise KeyError(f"quantize_block_mxfp4: tensor {name} is missing")
            current[name] = tensors[name].detach().to(dev).contiguous()
        return current[name]

    def run(g) -> Optional[torch.Tensor]:
        weights = {m: dev_t(m) for m in g.members}
        st = group_stats(q, stats, g)
        K = next(iter(weights.values())).shape[1]
        fold = g.foldable and st is not None
        if fold:
            out = q.quantize_layer_group_mxfp4(weights, x_mean=st[0], x_sq=st[1], scale_rule=scale_rule)
            for m, r in out["results"].items():
                results[m] = {k: v for k, v in r.items() if k != "input_scale"}
            s = out["input_scale"]
            report[g.name] = {"ratio": out["ratio"], "losses": out["losses"], "folded": True, "clip": None}
        else:
            for m, w in weights.items():
                results[m] = q.quantize_mxfp4(w, scale_rule)
            s = torch.ones(K, dtype=torch.float32, device=dev)
            report[g.name] = {"ratio": None, "losses": None, "folded": False, "clip": None}
        for m in g.members:
            scales[f"{m}.input_scale"] = s
        return s if fold else None

    groups = block.groups
    for gname in ("attn_out", "mlp_out"):
        g = groups.get(gname)
        s_out = run(g) if g is not None else None
        if s_out is None:
            continue
        pw = g.producers[0]
        current[pw] = _hip.fold_rows(dev_t(pw), s_out)            # a new device tensor: the source stays
        scales[f"{pw}.row_scale"] = s_out
        for pb in g.producers[1:]:
            folded[pb] = _hip.fold_rows(dev_t(pb), s_out)
    for gname in ("attn_in", "mlp_in"):
        g = groups.get(gname)
        s_in = run(g) if g is not None else None
        if s_in is not None:
            folded[g.producers[0]] = _hip.fold_rows(dev_t(g.producers[0]), s_in)
    return {"results": results, "folded": folded, "scales": scales, "groups": report}
