"""GPTQ error-compensated rounding (AWQQuantizer.quantize_gptq).

Round-to-nearest chooses every element's field on its own.  GPTQ (Frantar et al., 2022) rounds one
input column at a time and takes that column's error off the columns not yet rounded, through the
inverse of the Hessian H = X^T X of the layer's input, so that the error at the layer's OUTPUT on
the samples X shrinks.  With H^-1 = U^T U (U upper triangular) column c's error
e = (w_c - dq_c) / U[c][c] moves every later column j by -e U[c][j].

The dependent chain inside a block of 128 columns is one HIP kernel (include/awq_hip.h
awq_gptq_round_block: a lane per row, the block in registers); the Cholesky factorisations and the
update of the columns right of each block are torch.linalg / torch GEMMs on the device, as the
calibration forward's GEMMs are.  Group parameters are taken when the solver reaches a group's
first column, from the working values as they then stand (static groups, no act-order: g_idx stays
k // group_size).  The samples are those of the full-precision forward, as AWQ's are, not the
outputs of already quantized predecessors, as AutoGPTQ's are.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from .. import _hip
from ..layout import device_input

GPTQ_GROUP_SIZES = (32, 64, 128)
DAMP_TRIES = 3


def _factor(H: torch.Tensor, damp: float) -> Optional[torch.Tensor]:
    """U (fp32, upper, contiguous) with (H + damp mean(diag H) I)^-1 = U^T U, or None when a
    factorisation fails or leaves a non-finite value."""
    K = H.shape[0]
    Hd = H.clone()
    Hd.diagonal().add_(damp * float(H.diagonal().mean()))
    try:
        L = torch.linalg.cholesky(Hd)
        U = torch.linalg.cholesky(torch.cholesky_inverse(L), upper=True)
    except RuntimeError:                      # torch.linalg.LinAlgError is one
        return None
    if U.shape != (K, K) or not bool(torch.isfinite(U).all()):
        return None
    return U.contiguous()


def quantize_gptq(q, tensor: torch.Tensor, samples: Optional[torch.Tensor] = None, *,
                  hessian: Optional[torch.Tensor] = None, input_scale: Optional[torch.Tensor] = None,
                  damp: float = 0.01) -> Dict[str, torch.Tensor]:
    """AWQQuantizer.quantize_gptq (its docstring says what goes in and out)."""
    q._check_input(tensor)
    q._check_mode()
    if tensor.dim() != 2:
        raise ValueError("quantize_gptq takes a 2-D [out_features, in_features] weight")
    if tensor.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise ValueError(f"quantize_gptq takes bf16 / fp16 / fp32 weights, got {tensor.dtype}")
    N, K = tensor.shape
    L = q.group_size
    if L not in GPTQ_GROUP_SIZES or K % L or N == 0 or K == 0:
        raise ValueError(f"quantize_gptq needs group_size in {GPTQ_GROUP_SIZES} dividing in_features "
                         f"(group_size={L}, shape={tuple(tensor.shape)})")
    if samples is None and hessian is None:
        raise ValueError("quantize_gptq needs token samples (samples=) or a Hessian (hessian=)")
    if samples is not None and (not isinstance(samples, torch.Tensor) or samples.dim() != 2 or samples.shape[1] != K):
        raise ValueError(f"samples must be [tokens, {K}], got "
                         f"{tuple(samples.shape) if isinstance(samples, torch.Tensor) else type(samples)}")
    if hessian is not None and (not isinstance(hessian, torch.Tensor) or tuple(hessian.shape) != (K, K)):
        raise ValueError(f"hessian must be [{K}, {K}]")
    if isinstance(damp, bool) or not isinstance(damp, (int, float)) or not math.isfinite(damp) or not 0 < damp < 1:
        raise ValueError(f"damp must be a number in (0, 1): {damp!r}")
    if input_scale is not None and (not isinstance(input_scale, torch.Tensor) or input_scale.numel() != K):
        raise ValueError(f"input_scale must have in_features = {K} elements")

    dev = q.compute_device()
    w = device_input(tensor.detach(), dev)
    s = rs = None
    ws = w
    if input_scale is not None:
        s = input_scale.detach().to(dev, torch.float32).contiguous().reshape(K)
        rs = _hip.act_recip_table(s.reshape(1, K)).reshape(K)
        ws = _hip.apply_input_scale(w, s)
    xs = None
    if samples is not None:
        xs = device_input(samples.detach().to(w.dtype), dev)       # what awq_output_error reads: the unscaled inputs

    def output_loss(r) -> Optional[float]:
        if xs is None:
            return None
        err_sq, _, _ = _hip.output_error(w, L, q.bits, q.symmetric, r["qweight"], r["qzeros"], r["scales"], xs, s,
                                         ref=False)
        return float(err_sq.double().sum())

    if hessian is not None:
        H = hessian.detach().to(dev, torch.float32).clone()
    else:
        x32 = samples.detach().to(dev).float()
        if rs is not None:
            x32 = x32 * rs
        H = x32.t() @ x32
    rtn = q.quantize_packed(ws)
    loss_rtn = output_loss(rtn)
    diag = H.diagonal()
    dead = diag == 0
    n_dead = int(dead.sum())

    def fallback(why: str, used: float):
        q.logger.warning(f"quantize_gptq: {why}: rounding to nearest")
        return dict(rtn, rounding={"loss": loss_rtn, "loss_rtn": loss_rtn, "dead_columns": n_dead, "damp": used,
                                   "fallback": True}, **({"input_scale": s} if s is not None else {}))

    if not bool(torch.isfinite(ws).all()) or not bool(torch.isfinite(H).all()):
        return fallback("a non-finite weight or Hessian", float(damp))
    diag[dead] = 1.0
    work = ws.float().contiguous()
    if work.data_ptr() == ws.data_ptr():          # fp32 weights: the caller's tensor is not the working copy
        work = work.clone()
    work[:, dead] = 0.0
    U, used = None, float(damp)
    for attempt in range(DAMP_TRIES):
        U = _factor(H, used)
        if U is not None:
            break
        if attempt + 1 < DAMP_TRIES:
            used *= 10.0
    if U is None:
        return fallback(f"the Cholesky factorisation failed with damp up to {used:g}", used)

    from .awq import _alloc_packed
    r = _alloc_packed(q, tensor.shape, dev)
    r["qzeros"].zero_()                           # the kernel writes zero fields, not whole words
    for c0 in range(0, K, _hip.GPTQ_BLOCK):
        c1 = min(c0 + _hip.GPTQ_BLOCK, K)
        err = torch.empty((N, c1 - c0), dtype=torch.float32, device=dev)
        _hip.gptq_round_block(work, U, L, q.bits, q.symmetric, c0, c1 - c0, err, r["qweight"], r["qzeros"], r["scales"])
        if c1 < K:
            work[:, c1:].addmm_(err, U[c0:c1, c1:], alpha=-1.0)
    if s is not None:
        r["input_scale"] = s
    r["rounding"] = {"loss": output_loss(r), "loss_rtn": loss_rtn, "dead_columns": n_dead, "damp": used,
                     "fallback": False}
    return r
