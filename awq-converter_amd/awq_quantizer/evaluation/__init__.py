"""Model-level evaluation: how much worse is the written checkpoint than its source?

  compare_logits(ref, q=None, targets=None)           one fused pass over two logit matrices
  evaluate_model(model_dir, input_ids, quantized_dir)  perplexity of the source and, with a written
                                                       directory, of the quantized model, the KL
                                                       divergence between them and top-1 agreement

The forward is the calibration pass' block loop (calibration/forward.py run_decoder, statistics
off); the tail is here: final norm -> head GEMM -> awq_logit_compare, chunk by chunk, so the full
[n * seq, vocab] logits never exist.  Everything runs on the GPU through the HIP kernels; there is
no CPU fallback (_hip.HipUnavailable).  `ops` and `dequant` exist for host tests, which inject
float64 torch compositions.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from ..calibration import check_input_ids, resolve_dtype
from ..calibration.forward import HipOps, parse_config, read_config, run_decoder
from .checkpoint import DeviceDequant, QuantizedCheckpoint

__all__ = ["compare_logits", "evaluate_model", "aggregate", "shifted_targets", "HipEvalOps", "QuantizedCheckpoint",
           "DeviceDequant"]

def shifted_targets(input_ids: torch.Tensor) -> torch.Tensor:
    """[n, seq] ids -> int64 [n * seq]: the next token of the same sequence; -1 (not scored) at
    every sequence's last position."""
    t = torch.full_like(input_ids, -1)
    t[:, :-1] = input_ids[:, 1:]
    return t.reshape(-1)


def aggregate(per: Dict[str, torch.Tensor], targets: Optional[torch.Tensor]) -> dict:
    """The aggregates of per-token outputs (fp64 sums of the fp32 values).  per: nll_ref /
    argmax_ref, and nll_q / kl / argmax_q when a second model was compared; targets as the kernel
    took them (None: nothing is scored)."""
    n = int(per["argmax_ref"].numel())
    am_r = per["argmax_ref"].to(torch.int64)
    has_q = per.get("argmax_q") is not None
    bad = am_r < 0
    if has_q:
        am_q = per["argmax_q"].to(torch.int64)
        bad = bad | (am_q < 0)
    scored = (targets >= 0) if targets is not None else torch.zeros(n, dtype=torch.bool, device=am_r.device)
    ns = int(scored.sum())
    nan = float("nan")

    def ppl(nll_sum):
        if not ns:
            return nan
        try:
            return math.exp(nll_sum / ns)
        except OverflowError:
            return math.inf

    out = {"n_positions": n, "n_tokens_scored": ns, "nonfinite_rows": int(bad.sum())}
    nll_r = float(per["nll_ref"].double()[scored].sum()) if targets is not None and ns else 0.0
    out.update(nll_ref_sum=nll_r, ppl_ref=ppl(nll_r),
               top1_accuracy_ref=float((am_r == targets)[scored].double().mean()) if ns else nan)
    if has_q:
        nll_q = float(per["nll_q"].double()[scored].sum()) if targets is not None and ns else 0.0
        kl = per["kl"].double()
        out.update(nll_q_sum=nll_q, ppl_q=ppl(nll_q),
                   ppl_ratio=ppl(nll_q) / ppl(nll_r) if ns else nan,
                   kl_mean=float(kl.mean()) if n else nan, kl_max=float(kl.max()) if n else nan,
                   top1_agreement=float((am_r == am_q).double().mean()) if n else nan,
                   top1_accuracy_q=float((am_q == targets)[scored].double().mean()) if ns else nan)
    return out


def _device_compare(ref, q, targets) -> Dict[str, torch.Tensor]:
    from .. import _hip
    T, dev = ref.shape[0], ref.device
    out = {"nll_ref": torch.empty(T, dtype=torch.float32, device=dev) if targets is not None else None,
           "argmax_ref": torch.empty(T, dtype=torch.int32, device=dev), "nll_q": None, "kl": None, "argmax_q": None}
    if q is not None:
        out.update(nll_q=torch.empty(T, dtype=torch.float32, device=dev) if targets is not None else None,
                   kl=torch.empty(T, dtype=torch.float32, device=dev),
                   argmax_q=torch.empty(T, dtype=torch.int32, device=dev))
    _hip.logit_compare(ref, q, targets, **out)
    return out


def compare_logits(ref: torch.Tensor, q: Optional[torch.Tensor] = None,
                   targets: Optional[torch.Tensor] = None) -> dict:
    """ref, q: logits [T, V] (bf16 / fp16 / fp32, rows contiguous, any row stride) on the GPU;
    targets int64 [T] (< 0: not scored).  Returns the per-token tensors nll_ref, nll_q, kl (fp32),
    argmax_ref, argmax_q (int32; None where an input is missing) and aggregate()'s numbers
    (include/awq_hip.h awq_logit_compare defines every value)."""
    from .. import _hip
    _hip.require_device(ref.device)
    if targets is not None:
        targets = targets.to(ref.device, torch.int64).contiguous()
    per = _device_compare(ref, q, targets)
    return {**per, **aggregate(per, targets)}


class HipEvalOps(HipOps):
    """The calibration ops plus the fused comparison."""

    def logit_compare(self, ref, q, targets) -> Dict[str, torch.Tensor]:
        return _device_compare(ref, q, targets)


def _tail(cfg, loaders, hiddens, targets, dtype, device, ops, batch_tokens) -> Dict[str, torch.Tensor]:
    """final norm -> head -> comparison, per chunk of <= batch_tokens tokens.  loaders / hiddens:
    the source's, then (optionally) the quantized model's."""
    heads = []
    for loader in loaders:
        index = {i.name: i for i in loader.tensor_index()}
        root = "model." if "model.embed_tokens.weight" in index else ""
        head = "lm_head.weight" if "lm_head.weight" in index else f"{root}embed_tokens.weight"
        heads.append(tuple(loader.read(index[k]).to(device=device, dtype=dtype) for k in (f"{root}norm.weight", head)))
    N = hiddens[0].shape[0]
    outs = {}
    for a in range(0, N, batch_tokens):
        b = min(a + batch_tokens, N)
        logits = [F.linear(ops.rmsnorm(h[a:b], wn, cfg.eps, None, False), wh) for h, (wn, wh) in zip(hiddens, heads)]
        per = ops.logit_compare(logits[0], logits[1] if len(logits) > 1 else None, targets[a:b])
        for k, v in per.items():
            if v is not None:
                outs.setdefault(k, []).append(v)
    return {k: torch.cat(v) for k, v in outs.items()}


def evaluate_model(model_dir: str, input_ids, quantized_dir: Optional[str] = None, compute_dtype=None,
                   batch_tokens: int = 8192, device="cuda", logger=None, ops=None, dequant=None,
                   per_token: Optional[Dict[str, torch.Tensor]] = None) -> dict:
    """Perplexity of the model in model_dir on input_ids [n, seq] (targets: the next token of the
    same sequence; every sequence's last position is not scored) and, with quantized_dir (any
    directory main wrote), of the quantized model, with KL(source || quantized) and the top-1
    agreement over every position.  Returns n_tokens_scored, n_positions, nll_ref_sum, ppl_ref,
    top1_accuracy_ref, nonfinite_rows, and with quantized_dir nll_q_sum, ppl_q, ppl_ratio, kl_mean,
    kl_max, top1_agreement, top1_accuracy_q.  per_token, when a dict, receives the per-token
    tensors (CPU).  compute_dtype: the checkpoint's by default."""
    from ..model_loading.safetensors_loader import SafetensorsLoader
    ids = check_input_ids(input_ids)
    if batch_tokens <= 0:
        raise ValueError("batch_tokens must be positive")
    cfg = parse_config(read_config(model_dir), seq_len=ids.shape[1], max_id=int(ids.max()))   # before the model is read
    device = torch.device(device)
    if ops is None:
        ops = HipEvalOps(device)
    loader = SafetensorsLoader(model_dir, logger_level="WARNING")
    qloader = None
    try:
        index = {i.name: i for i in loader.tensor_index()}
        embed = index.get("model.embed_tokens.weight") or index.get("embed_tokens.weight")
        dtype = resolve_dtype(compute_dtype, embed.dtype if embed is not None else None)
        if isinstance(ops, HipOps) and dtype == torch.float64:
            raise ValueError("compute_dtype float64: the kernels take bfloat16 / float16 / float32")
        loaders = [loader]
        if quantized_dir is not None:
            qloader = QuantizedCheckpoint(loader, quantized_dir, dequant or DeviceDequant(device))
            loaders.append(qloader)
        hiddens = []
        with torch.no_grad():
            for ld in loaders:
                got: Dict[str, torch.Tensor] = {}
                run_decoder(ld, cfg, ids, dtype, device, ops, batch_tokens=batch_tokens, logger=logger, stats=False,
                            hidden_out=got)
                hiddens.append(got["hidden"])
            targets = shifted_targets(ids).to(device)
            per = _tail(cfg, loaders, hiddens, targets, dtype, device, ops, batch_tokens)
        if per_token is not None:
            per_token.update({k: v.cpu() for k, v in per.items()})
            per_token["targets"] = targets.cpu()
        return aggregate(per, targets)
    finally:
        if qloader is not None:
            qloader.close()
        loader.close()
