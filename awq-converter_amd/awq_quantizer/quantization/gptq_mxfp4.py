"""GPTQ error-compensated rounding onto the MXFP4 grid (AWQQuantizer.quantize_gptq_mxfp4).

gptq_round.py's solve with another grid: a block of 32 input columns takes its power-of-two scale,
by quantize_mxfp4's rule, from the working values as they stand when the solver reaches its first
column; each column is rounded to the nearest E2M1 magnitude and its error e = (w_c - dq_c) / U[c][c]
moves every later column j by -e U[c][j] (H^-1 = U^T U).  The dependent chain inside a call of 128
columns is one HIP kernel (include/awq_hip.h awq_gptq_round_block_mxfp4: a quad of lanes per row, a
block per lane); the update of the columns right of each call is a torch GEMM on the device, as in
quantize_gptq.  The factor is gptq_round._factor's, so q.gptq_factor is honoured.

No act_order: MXFP4 has no g_idx, and a block of permuted columns is not a block a reader finds in
the row.  No input_scale: folding a searched scale into MXFP4 weights stays refused.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from .. import _hip
from ..layout import device_input
from . import mxfp4
from .gptq_round import DAMP_TRIES, GPTQ_FACTORS, _factor


def check_inputs(q, tensor, samples, hessian, scale_rule, damp) -> str:
    """Everything quantize_gptq_mxfp4 refuses, before the device is touched.  -> q.gptq_factor."""
    mxfp4.check_weight(tensor)
    N, K = tensor.shape
    if N == 0 or K == 0:
        raise ValueError(f"quantize_gptq_mxfp4 takes a non-empty weight, got {tuple(tensor.shape)}")
    if scale_rule not in mxfp4.SCALE_RULES:
        raise ValueError(f"scale_rule must be one of {list(mxfp4.SCALE_RULES)}, got {scale_rule!r}")
    if isinstance(damp, bool) or not isinstance(damp, (int, float)) or not math.isfinite(damp) or not 0 < damp < 1:
        raise ValueError(f"damp must be a number in (0, 1): {damp!r}")
    if samples is None and hessian is None:
        raise ValueError("quantize_gptq_mxfp4 needs token samples (samples=) or a Hessian (hessian=)")
    if samples is not None and (not isinstance(samples, torch.Tensor) or samples.dim() != 2 or samples.shape[1] != K):
        raise ValueError(f"samples must be [tokens, {K}], got "
                         f"{tuple(samples.shape) if isinstance(samples, torch.Tensor) else type(samples)}")
    if hessian is not None and (not isinstance(hessian, torch.Tensor) or tuple(hessian.shape) != (K, K)):
        raise ValueError(f"hessian must be [{K}, {K}]")
    how = getattr(q, "gptq_factor", "torch")
    if how not in GPTQ_FACTORS:
        raise ValueError(f"gptq_factor must be one of {GPTQ_FACTORS}: {how!r}")
    return how


def prepare(H: torch.Tensor, damp: float, how: str):
    """The dead-column fix on H (in place: diag 0 -> 1) and up to DAMP_TRIES factorisations.
    -> (U or None, the damp used, dead [K] bool).  The caller has checked that H is finite."""
    diag = H.diagonal()
    dead = diag == 0
    diag[dead] = 1.0
    U, used = None, float(damp)
    for attempt in range(DAMP_TRIES):
        U = _factor(H, used, how)
        if U is not None:
            break
        if attempt + 1 < DAMP_TRIES:
            used *= 10.0
    return U, used, dead


def output_loss(q, result: dict, w: torch.Tensor, xs: Optional[torch.Tensor]) -> Optional[float]:
    """sum(((dq - w) X^T)^2): dq the fp32 dequantized result, the difference in fp32, the product and
    the sum in float64 on the device.  None without samples."""
    if xs is None:
        return None
    d = (mxfp4.dequantize_mxfp4(q, result, torch.float32) - w.float()).double()
    return float((d @ xs.double().t()).square().sum())


def solve(q, w: torch.Tensor, U: torch.Tensor, dead: torch.Tensor, scale_rule: str) -> Dict[str, torch.Tensor]:
    """The solver proper: w [N, K] on the device against the factor U -> an MXFP4 result."""
    N, K = w.shape
    dev = w.device
    work = w.float().contiguous()
    if work.data_ptr() == w.data_ptr():           # fp32 weights: the caller's tensor is not the working copy
        work = work.clone()
    work[:, dead] = 0.0
    codes = torch.empty((N, K // 2), dtype=torch.uint8, device=dev)
    scales = torch.empty((N, K // mxfp4.BLOCK), dtype=torch.uint8, device=dev)
    for c0 in range(0, K, _hip.GPTQ_BLOCK):
        c1 = min(c0 + _hip.GPTQ_BLOCK, K)
        err = torch.empty((N, c1 - c0), dtype=torch.float32, device=dev)
        _hip.gptq_round_block_mxfp4(work, U, scale_rule, c0, c1 - c0, err, codes, scales)
        if c1 < K:
            work[:, c1:].addmm_(err, U[c0:c1, c1:], alpha=-1.0)
    return {"codes": codes, "scales": scales, "format": mxfp4.FORMAT, "scale_rule": scale_rule,
            "shape": torch.tensor([N, K], dtype=torch.int64)}


def quantize_gptq_mxfp4(q, tensor: torch.Tensor, samples: Optional[torch.Tensor] = None, *,
                        hessian: Optional[torch.Tensor] = None, scale_rule: str = "floor", damp: float = 0.01,
                        factor=None) -> Dict[str, torch.Tensor]:
    """AWQQuantizer.quantize_gptq_mxfp4 (its docstring says what goes in and out).  factor: a
    prepare() result for this input's Hessian, shared by the linears of a layer group (the CLI)."""
    how = check_inputs(q, tensor, samples, hessian, scale_rule, damp)
    dev = q.compute_device()
    w = device_input(tensor.detach(), dev)
    xs = device_input(samples.detach().to(w.dtype), dev) if samples is not None else None
    rtn = mxfp4.quantize_mxfp4(q, w, scale_rule)
    loss_rtn = output_loss(q, rtn, w, xs)

    def fallback(why: str, used: float, n_dead: int):
        q.logger.warning(f"quantize_gptq_mxfp4: {why}: rounding to nearest")
        return dict(rtn, rounding={"loss": loss_rtn, "loss_rtn": loss_rtn, "dead_columns": n_dead, "damp": used,
                                   "fallback": True, "factor": how})

    if factor is None:
        if hessian is not None:
            H = hessian.detach().to(dev, torch.float32).clone()
        else:
            x32 = samples.detach().to(dev).float()
            H = x32.t() @ x32
        if not bool(torch.isfinite(H).all()):
            return fallback("a non-finite Hessian", float(damp), int((H.diagonal() == 0).sum()))
        factor = prepare(H, damp, how)
    U, used, dead = factor
    n_dead = int(dead.sum())
    if not bool(torch.isfinite(w).all()):
        return fallback("a non-finite weight", float(damp), n_dead)
    if U is None:
        return fallback(f"the Cholesky factorisation failed with damp up to {used:g}", used, n_dead)
    r = solve(q, w, U, dead, scale_rule)
    r["rounding"] = {"loss": output_loss(q, r, w, xs), "loss_rtn": loss_rtn, "dead_columns": n_dead, "damp": used,
                     "fallback": False, "factor": how}
    return r
