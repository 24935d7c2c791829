"""Activation-aware per-input-channel scale search (scale_method="awq").

No reference counterpart: the reference stores scale_method and never reads it
(awq.py:66,111-112) and collects no activations (SURVEY.md §8a, §8f row 4 — parity with
AutoAWQ unpinned).  The search and its canonical arithmetic are defined in
include/awq_hip.h (awq_act_*); every step below is one HIP launch through that ABI and
the CPU restatement is oracle/awq_oracle.c (oracle_act_*), used only by the tests.

For one layer group — linears W_j [R_j, K] that read the same input x [tokens, K]
(e.g. q/k/v projections) — candidate i scales input channel k by
s_i[k] ∝ x_mean[k]^r / (w_mean[k]^(1-r) + 1e-4) (r = i / n_grid; without duo scaling
x_mean[k]^r), quantizes W·diag(s_i), undoes s_i, and scores the result with
Σ_k E[x_k²] Σ_n (Ŵ - W)²_nk, the diagonal form of AutoAWQ's output MSE.  The winner's
W·diag(s) is quantized with the regular kernels and s is returned so the caller folds
1/s into whatever produces x (a norm's weight, the previous linear's rows).

search_layer_group is the search alone.  The functions that take the quantizer `q` are
AWQQuantizer's quantize_layer_group (with its output-space search and clip step) and
quantize_block; the methods' docstrings say what they take and return.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .. import _hip
from ..layout import aligned, device_input

ACT_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _check_group(weights: Dict[str, torch.Tensor], group_size: int):
    if not weights:
        raise ValueError("quantize_layer_group needs at least one weight")
    Ks = {tuple(w.shape[1:]) for w in weights.values()}
    dts = {w.dtype for w in weights.values()}
    for name, w in weights.items():
        if not isinstance(w, torch.Tensor) or w.dim() != 2:
            raise ValueError(f"{name}: activation-aware search takes 2-D [out_features, in_features] weights")
    if len(Ks) != 1:
        raise ValueError("all weights of a layer group must share in_features (they read the same input)")
    if len(dts) != 1 or next(iter(dts)) not in ACT_DTYPES:
        raise ValueError(f"weights of a layer group must share one dtype of {ACT_DTYPES}, got {sorted(map(str, dts))}")
    K = next(iter(Ks))[0]
    if group_size < 8 or group_size > 512 or group_size & (group_size - 1) or K % group_size:
        raise ValueError(f"activation-aware search needs a power-of-two group_size in [8, 512] dividing "
                         f"in_features (group_size={group_size}, in_features={K})")
    return K


def search_layer_group(weights: Dict[str, torch.Tensor], device: torch.device, *, group_size: int, bits: int,
                       symmetric: bool, n_grid: int, duo_scaling: bool,
                       activations: Optional[torch.Tensor] = None, x_mean: Optional[torch.Tensor] = None,
                       x_sq: Optional[torch.Tensor] = None, table: Optional[torch.Tensor] = None,
                       scale_weights: bool = True) -> dict:
    """Run the search on the device; returns device tensors
    {"x_mean", "x_sq", "w_mean", "table", "losses", "best", "input_scale", "weights": {name: W on
    the device}, "scaled": {name: W·diag(s)} (None with scale_weights=False: the caller
    quantizes W·diag(s) in one pass, awq_quantize_groups_scaled)}.
    `table` overrides the scale table (a caller's own table; since round 5 the kernel's table
    is bit-exact with the oracle's from the inputs alone, include/awq_hip.h awq_pow)."""
    K = _check_group(weights, group_size)
    if not 1 <= n_grid <= _hip.ACT_MAX_GRID:
        raise ValueError(f"search_grid must be in [1, {_hip.ACT_MAX_GRID}] for scale_method='awq': {n_grid}")
    ws = [w.detach().to(device).contiguous() for w in weights.values()]
    if activations is not None:
        if activations.dim() != 2 or activations.shape[1] != K or activations.dtype not in ACT_DTYPES:
            raise ValueError(f"activations must be [tokens, {K}] bf16/fp16/fp32, got {tuple(activations.shape)} "
                             f"{activations.dtype}")
        x_mean, x_sq = _hip.act_stats(activations.detach().to(device).contiguous())
    elif x_mean is None or x_sq is None:
        raise ValueError("scale_method='awq' needs calibration activations, or both x_mean and x_sq")
    else:
        if x_mean.numel() != K or x_sq.numel() != K:
            raise ValueError(f"x_mean / x_sq must have in_features = {K} elements")
        x_mean = x_mean.detach().to(device, torch.float32).contiguous().reshape(K)
        x_sq = x_sq.detach().to(device, torch.float32).contiguous().reshape(K)
    w_mean = _hip.weight_mean(ws, group_size) if duo_scaling else None
    if table is None:
        table = _hip.act_scale_table(x_mean, w_mean, n_grid)
    else:
        table = table.detach().to(device, torch.float32).contiguous()
        if tuple(table.shape) != (n_grid, K):
            raise ValueError(f"table must be [{n_grid}, {K}]")
    part = _hip.act_search_losses(ws, x_sq, table, group_size, bits, symmetric)
    losses, best, s_best = _hip.act_search_select(part, table)
    scaled = {name: _hip.apply_input_scale(w, s_best) for name, w in zip(weights, ws)} if scale_weights else None
    return {"x_mean": x_mean, "x_sq": x_sq, "w_mean": w_mean, "table": table, "losses": losses, "best": best,
            "input_scale": s_best, "weights": dict(zip(weights, ws)), "scaled": scaled}


def _check_args(q, what: str, loss: str, clip_loss: Optional[str] = None) -> str:
    """What quantize_layer_group and quantize_block refuse first.  -> the clip loss: the argument,
    or, when it is None, the quantizer's clip_loss attribute (AWQQuantizer's methods pass None)."""
    if q.scale_method != "awq":
        raise ValueError(f"{what} needs scale_method='awq'")
    if loss not in ("diag", "output"):
        raise ValueError(f"loss must be 'diag' or 'output': {loss!r}")
    if clip_loss is None:
        clip_loss = getattr(q, "clip_loss", "diag")
    if clip_loss not in ("diag", "output"):
        raise ValueError(f"clip_loss must be 'diag' or 'output': {clip_loss!r}")
    return clip_loss


def _check_rounding(q, what: str, clip: bool) -> bool:
    """The quantizer's rounding attribute ("nearest" / "gptq"; AWQQuantizer's methods have no such
    argument).  -> whether the groups with token samples take quantize_gptq."""
    rounding = getattr(q, "rounding", "nearest")
    if rounding not in ("nearest", "gptq"):
        raise ValueError(f"rounding must be 'nearest' or 'gptq': {rounding!r}")
    if rounding == "gptq" and clip:
        raise ValueError(f"{what}: clip=True with rounding='gptq': the solver moves the ranges the clip search chose")
    return rounding == "gptq"


def _log_rounding(q, name: str, r: dict) -> None:
    rd = r["rounding"]
    if rd["loss"] is not None:
        q.logger.info(f"gptq rounding {name}: output error {rd['loss_rtn']:.6g} -> {rd['loss']:.6g}, damp {rd['damp']:g}"
                      f"{', fallback to nearest' if rd['fallback'] else ''}")


def _quantize_scaled(q, w: torch.Tensor, s: torch.Tensor, one_pass: bool, out: Optional[dict] = None,
                     scaled: Optional[torch.Tensor] = None) -> dict:
    """W * diag(s) as a quantize_packed() result.  `one_pass` (the shape is scaled_eligible) and a
    16-B aligned base: awq_quantize_groups_scaled, the scaled copy is never written, into `out`
    (an earlier return value whose buffers are reused) or fresh buffers.  Otherwise the copy
    (`scaled`, if the caller has it), then quantize_packed."""
    if one_pass and w.data_ptr() % 16 == 0:
        r = out if out is not None else q._packed_outputs(w)
        _hip.quantize_groups_scaled(w, s, q.group_size, q.bits, q.symmetric,
                                    qweight=r["qweight"], qzeros=r["qzeros"], scales=r["scales"])
        return r
    return q.quantize_packed(scaled if scaled is not None else _hip.apply_input_scale(w, s))


def quantize_layer_group(q, weights: Dict[str, torch.Tensor], activations: Optional[torch.Tensor] = None,
                         *, x_mean: Optional[torch.Tensor] = None, x_sq: Optional[torch.Tensor] = None,
                         packed: bool = True, table: Optional[torch.Tensor] = None, clip: bool = False,
                         clip_grid: int = 20, clip_max_shrink: float = 0.5, loss: str = "diag",
                         samples: Optional[torch.Tensor] = None, clip_loss: Optional[str] = None) -> dict:
    """The search over one layer group, then its weights quantized as W * diag(input_scale).
    clip_loss (with clip=True): "diag", the clip search's x_sq-weighted loss
    (awq_quantize_clip_scaled), or "output", every shrink of every group scored by the error at the
    linear's output on the token samples (awq_quantize_clip_output; samples=, default
    `activations`); None: the quantizer's clip_loss attribute.  The "clip" dict of an "output" run
    has the same keys plus "loss": "output", its losses are output-space losses."""
    clip_loss = _check_args(q, "quantize_layer_group", loss, clip_loss)
    gptq = _check_rounding(q, "quantize_layer_group", clip)
    gptq_samples = None
    if gptq:
        if not packed:
            raise ValueError("rounding='gptq' writes packed outputs only (packed=False is not available)")
        gptq_samples = activations if samples is None else samples
        if gptq_samples is None:
            q.logger.warning(f"rounding='gptq' without token samples for {list(weights)}: rounding to nearest")
    if loss == "output":
        samples = activations if samples is None else samples
        if samples is None:
            raise ValueError("loss='output' needs token samples (samples=, or activations=)")
    clip_samples = None
    if clip and clip_loss == "output":
        clip_samples = activations if samples is None else samples
        if clip_samples is None:
            raise ValueError("clip_loss='output' needs token samples (samples=, or activations=)")
    n_clip = 0
    if clip:
        if not packed:
            raise ValueError("clip=True writes packed outputs only (packed=False is not available)")
        if isinstance(clip_grid, bool) or not isinstance(clip_grid, int) or clip_grid < 1:
            raise ValueError(f"clip_grid must be a positive integer: {clip_grid}")
        if not 0.0 <= float(clip_max_shrink) <= 1.0:
            raise ValueError(f"clip_max_shrink must be in [0, 1]: {clip_max_shrink}")
        n_clip = min(clip_grid, max(1, int(clip_max_shrink * clip_grid)))
    _check_group(weights, q.group_size)
    q._check_mode()
    dev = q.compute_device()
    # packed outputs of eligible shapes take _quantize_scaled's one pass: the search need not write the copies
    one_pass = packed and (clip or all(
        _hip.scaled_eligible(w.dtype, w.shape[0], w.shape[1], q.group_size) for w in weights.values()))
    sr = search_layer_group(weights, dev, group_size=q.group_size, bits=q.bits, symmetric=q.symmetric,
                            n_grid=q.search_grid, duo_scaling=q.duo_scaling, activations=activations,
                            x_mean=x_mean, x_sq=x_sq, table=table,
                            scale_weights=not one_pass and gptq_samples is None)
    extra = {}
    if loss == "output":
        sr = output_search(q, sr, samples)
        extra = {"loss": "output", "diag_losses": sr["diag_losses"], "diag_best": int(sr["diag_best"].item())}
    if clip:
        return dict(clip_layer_group(q, weights, sr, clip_grid, n_clip, samples=clip_samples), **extra)
    results, s, scaled = {}, sr["input_scale"], sr["scaled"] or {}
    for name in weights:
        w = sr["weights"][name]
        if gptq_samples is not None:              # the solver scales the weight and the samples itself
            r = q.quantize_gptq(w, gptq_samples, input_scale=s, damp=getattr(q, "gptq_damp", 0.01))
            _log_rounding(q, name, r)
        elif packed:
            r = _quantize_scaled(q, w, s, one_pass, scaled=scaled.get(name))
        else:                                     # RTN of W * diag(s), the reference's result dict
            r = q._quantize_device(scaled[name] if name in scaled else _hip.apply_input_scale(w, s))
        r["input_scale"] = s
        results[name] = r
    best = int(sr["best"].item())
    q.logger.info(f"awq search over {list(weights)}: ratio {best}/{q.search_grid}")
    return dict({"results": results, "input_scale": s, "best": best,
                 "ratio": best / q.search_grid, "losses": sr["losses"], "table": sr["table"]}, **extra)


def output_search(q, sr: dict, samples: torch.Tensor) -> dict:
    """quantize_layer_group's loss="output": the search result `sr` with losses / best /
    input_scale taken from the output error on the samples.  Candidate i of every weight:
    awq_quantize_groups_scaled(w, table[i]) into the weight's reused packed buffer (the
    apply + quantize pair where that kernel does not take the shape), then awq_output_error
    with col_scale = table[i] writes the rows' sums into part[i, offset : offset + N];
    awq_act_search_select adds each candidate's row in fp64 and picks the first minimum."""
    table = sr["table"]
    n_grid, K = table.shape
    ws = sr["weights"]
    dev = table.device
    if samples.dim() != 2 or samples.shape[1] != K:
        raise ValueError(f"samples must be [tokens, {K}], got {tuple(samples.shape)}")
    dtype = next(iter(ws.values())).dtype
    xs = device_input(samples.detach().to(dtype), dev)
    part = torch.empty((n_grid, sum(w.shape[0] for w in ws.values())), dtype=torch.float32, device=dev)
    off = 0
    for w in ws.values():
        N = w.shape[0]
        one_pass = _hip.scaled_eligible(w.dtype, N, K, q.group_size)
        r = None                  # (one pass: the first candidate's buffers take the others too)
        for i in range(n_grid):
            r = _quantize_scaled(q, w, table[i], one_pass, out=r)
            _hip.output_error(w, q.group_size, q.bits, q.symmetric, aligned(r["qweight"]), r["qzeros"],
                              r["scales"], xs, table[i], ref=False, err_sq=part[i, off:off + N])
        off += N
    losses, best, s_best = _hip.act_search_select(part, table)
    return dict(sr, losses=losses, best=best, input_scale=s_best, scaled=None,
                diag_losses=sr["losses"], diag_best=sr["best"])


def clip_layer_group(q, weights, sr: dict, clip_grid: int, n_clip: int,
                     samples: Optional[torch.Tensor] = None) -> dict:
    """quantize_layer_group's last step with clip=True: every weight through
    awq_quantize_clip_scaled with the search's input scale, its reciprocals and x_sq — or, with
    token samples (clip_loss="output"), through awq_quantize_clip_output with the samples in
    x_sq's place; the groups' losses of all weights meet in one [2, total groups] buffer, summed
    in fp64 by awq_act_search_select (before = candidate 0, after = the winners)."""
    s, x_sq = sr["input_scale"], sr["x_sq"]
    K = s.numel()
    xs = None
    if samples is not None:
        if samples.dim() != 2 or samples.shape[1] != K:
            raise ValueError(f"samples must be [tokens, {K}], got {tuple(samples.shape)}")
        xs = device_input(samples.detach().to(next(iter(sr["weights"].values())).dtype), s.device)
    how = "diag" if xs is None else "output"
    G = K // q.group_size
    rs = _hip.act_recip_table(s.reshape(1, K)).reshape(K)
    names = list(weights)
    counts = [sr["weights"][n].shape[0] * G for n in names]
    loss = torch.empty((2, sum(counts)), dtype=torch.float32, device=s.device)
    results, idx, off = {}, {}, 0
    for name, cnt in zip(names, counts):
        w = sr["weights"][name]
        r = q._packed_outputs(w)
        idx[name] = torch.empty(cnt, dtype=torch.int32, device=s.device)
        if xs is None:
            _hip.quantize_clip_scaled(w, s, x_sq, q.group_size, q.bits, q.symmetric, clip_grid, n_clip,
                                      rscale=rs, qweight=r["qweight"], qzeros=r["qzeros"], scales=r["scales"],
                                      best_idx=idx[name], group_loss=loss, loss_offset=off)
        else:
            _hip.quantize_clip_output(w, s, xs, q.group_size, q.bits, q.symmetric, clip_grid, n_clip,
                                      rscale=rs, qweight=r["qweight"], qzeros=r["qzeros"], scales=r["scales"],
                                      best_idx=idx[name], group_loss=loss, loss_offset=off)
        r["input_scale"] = s
        results[name] = r
        off += cnt
    # (the select kernel also copies the winning row of a table: two rows of s keep that in range)
    two = s.reshape(1, K).expand(2, K).contiguous()
    total, _, _ = _hip.act_search_select(loss, two)
    total = total.cpu()
    per, off, clipped = {}, 0, 0
    for name, cnt in zip(names, counts):
        one, _, _ = _hip.act_search_select(loss[:, off:off + cnt].contiguous(), two)
        one = one.cpu()
        nz = int((idx[name] != 0).sum().item())
        per[name] = {"loss_before": float(one[0]), "loss_after": float(one[1]), "clipped_fraction": nz / cnt}
        q.logger.info(f"awq clip {name}: clipped {nz / cnt:.1%} of {cnt} groups, {how} loss "
                         f"{float(one[0]):.6g} -> {float(one[1]):.6g}")
        clipped += nz
        off += cnt
    best = int(sr["best"].item())
    q.logger.info(f"awq search over {names}: ratio {best}/{q.search_grid}, clip {n_clip}/{clip_grid}")
    clip = {"loss_before": float(total[0]), "loss_after": float(total[1]),
            "clipped_fraction": clipped / sum(counts), "per_weight": per, "best_idx": idx}
    if xs is not None:
        clip["loss"] = "output"
    return {"results": results, "input_scale": s, "best": best, "ratio": best / q.search_grid,
            "losses": sr["losses"], "table": sr["table"], "clip": clip}


def quantize_block(q, tensors: Dict[str, torch.Tensor], stats: Dict[str, Tuple[torch.Tensor, torch.Tensor]],
                   block, *, clip: bool = False, clip_grid: int = 20, clip_max_shrink: float = 0.5,
                   samples: Optional[Dict[str, torch.Tensor]] = None, loss: str = "diag",
                   clip_loss: Optional[str] = None) -> dict:
    """One decoder block: the out groups, their row folds, the in groups, their norm folds.
    clip_loss="output" (with clip=True): every group with token samples takes the output-space clip
    loss, folded or not; a group without samples the diagonal one, with a warning."""
    clip_loss = _check_args(q, "quantize_block", loss, clip_loss)
    gptq = _check_rounding(q, "quantize_block", clip)
    q._check_mode()
    dev = q.compute_device()
    clip_kw = {"clip": True, "clip_grid": clip_grid, "clip_max_shrink": clip_max_shrink} if clip else {}
    results, folded, scales, report = {}, {}, {}, {}
    current: Dict[str, torch.Tensor] = {}     # device tensors, row-folded producers replaced

    def dev_t(name: str) -> torch.Tensor:
        if name not in current:
            if name not in tensors:
                raise KeyError(f"quantize_block: tensor {name} is missing")
            current[name] = tensors[name].detach().to(dev).contiguous()
        return current[name]

    def group_stats(g):
        have = [m for m in g.members if m in stats]
        if not have:
            return None
        first = stats[have[0]]
        for m in have[1:]:
            if not (torch.equal(stats[m][0], first[0]) and torch.equal(stats[m][1], first[1])):
                q.logger.warning(f"{m}: activation statistics differ from {have[0]}'s (same input): "
                                    f"using {have[0]}'s for the {g.name} group")
        return first

    def run(g) -> Optional[torch.Tensor]:
        weights = {m: dev_t(m) for m in g.members}
        st = group_stats(g)
        K = next(iter(weights.values())).shape[1]
        fold = g.foldable and st is not None
        if fold or (clip and st is not None):
            table = None if fold else torch.ones((q.search_grid, K), dtype=torch.float32, device=dev)
            loss_kw = {}
            if fold and loss == "output":
                smp = (samples or {}).get(g.name)
                if smp is None:
                    q.logger.warning(f"{g.name}: no token samples for loss='output': diagonal loss")
                else:
                    loss_kw = {"loss": "output", "samples": smp}
            how = "diag"
            if clip and clip_loss == "output":
                smp = (samples or {}).get(g.name)
                if smp is None:
                    q.logger.warning(f"{g.name}: no token samples for clip_loss='output': diagonal loss")
                else:
                    how = "output"
                    loss_kw["samples"] = smp
            if gptq and (samples or {}).get(g.name) is not None:
                loss_kw["samples"] = samples[g.name]
            if how == getattr(q, "clip_loss", "diag"):    # the method resolves to the same choice: the call as it
                out = q.quantize_layer_group(weights, x_mean=st[0], x_sq=st[1], table=table, **clip_kw, **loss_kw)
            else:                                         # was (an override of the method is honoured)
                out = quantize_layer_group(q, weights, x_mean=st[0], x_sq=st[1], table=table, **clip_kw, **loss_kw,
                                           clip_loss=how)
            for m, r in out["results"].items():
                results[m] = {k: v for k, v in r.items() if k not in ("input_scale", "rounding")}
            s = out["input_scale"]
            report[g.name] = {"ratio": out["ratio"] if fold else None, "losses": out["losses"] if fold else None,
                              "folded": fold, "clip": out.get("clip")}
            if gptq:
                report[g.name]["rounding"] = {m: r["rounding"] for m, r in out["results"].items() if "rounding" in r}
            if loss_kw.get("loss"):
                report[g.name].update(loss="output", best=out["best"], diag_best=out["diag_best"])
        else:
            smp = (samples or {}).get(g.name) if gptq else None
            if gptq and smp is None:
                q.logger.warning(f"{g.name}: no token samples for rounding='gptq': rounding to nearest")
            report[g.name] = {"ratio": None, "losses": None, "folded": False, "clip": None}
            for m, w in weights.items():
                if smp is None:
                    results[m] = q.quantize_packed(w)
                    continue
                r = q.quantize_gptq(w, smp, damp=getattr(q, "gptq_damp", 0.01))
                _log_rounding(q, m, r)
                report[g.name].setdefault("rounding", {})[m] = r.pop("rounding")
                results[m] = r
            s = torch.ones(K, dtype=torch.float32, device=dev)
        for m in g.members:
            scales[f"{m}.input_scale"] = s
        return s if fold else None

    groups = block.groups
    for gname in ("attn_out", "mlp_out"):
        g = groups.get(gname)
        if g is None:
            continue
        s_out = run(g)
        if s_out is None:
            continue
        pw = g.producers[0]
        current[pw] = _hip.fold_rows(dev_t(pw), s_out)            # a new device tensor: the source stays
        scales[f"{pw}.row_scale"] = s_out
        for pb in g.producers[1:]:
            folded[pb] = _hip.fold_rows(dev_t(pb), s_out)
    for gname in ("attn_in", "mlp_in"):
        g = groups.get(gname)
        if g is None:
            continue
        s_in = run(g)
        if s_in is not None:
            folded[g.producers[0]] = _hip.fold_rows(dev_t(g.producers[0]), s_in)
    return {"results": results, "folded": folded, "scales": scales, "groups": report}
