"""MXFP4 weights (OCP microscaling FP4; include/awq_hip.h awq_quantize_mxfp4) behind
AWQQuantizer.quantize_mxfp4 / dequantize_mxfp4 and the quantization_error of such a result.

A result: {"codes": uint8 [N, K / 2] (two E2M1 codes per byte, the even element in the low nibble),
"scales": uint8 [N, K / 32] (E8M0: 2^(e - 127), 255 = NaN), "format": "mxfp4", "shape": int64 [2],
"scale_rule": "floor" | "ceil" | "mse"}, codes and scales on the compute device.  The format fixes
the block (32 along K) and the element type, so the quantizer's bits, group_size and symmetric are
not consulted anywhere in this module.
"""
from typing import Dict

import torch

from .. import _hip
from ..layout import device_input
from .report import error_report

BLOCK = 32
FORMAT = "mxfp4"
SCALE_RULES = tuple(_hip.MXFP4_RULES)
DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def check_weight(tensor: torch.Tensor) -> None:
    if not isinstance(tensor, torch.Tensor) or tensor.dim() != 2:
        raise ValueError("mxfp4 takes a 2-D weight [out_features, in_features]")
    if tensor.dtype not in DTYPES:
        raise ValueError(f"mxfp4 takes bf16 / fp16 / fp32 weights, got {tensor.dtype}")
    if tensor.shape[1] % BLOCK != 0:
        raise ValueError(f"mxfp4 needs in_features % {BLOCK} == 0, got a weight {tuple(tensor.shape)}")


def quantize_mxfp4(q, tensor: torch.Tensor, scale_rule: str = "floor") -> Dict[str, torch.Tensor]:
    """tensor [N, K] -> an MXFP4 result on the compute device (the module's docstring)."""
    check_weight(tensor)
    if scale_rule not in SCALE_RULES:
        raise ValueError(f"scale_rule must be one of {list(SCALE_RULES)}, got {scale_rule!r}")
    dev = q.compute_device()
    x = device_input(tensor, dev)
    N, K = x.shape
    codes = torch.empty((N, K // 2), dtype=torch.uint8, device=dev)
    scales = torch.empty((N, K // BLOCK), dtype=torch.uint8, device=dev)
    _hip.quantize_mxfp4(x, scale_rule, codes, scales)
    return {"codes": codes, "scales": scales, "format": FORMAT, "scale_rule": scale_rule,
            "shape": torch.tensor([N, K], dtype=torch.int64)}


def stored_result(codes: torch.Tensor, scales: torch.Tensor) -> Dict[str, torch.Tensor]:
    """`<prefix>.weight` / `<prefix>.weight_scale` of a written directory as a quantize_mxfp4 result."""
    return {"codes": codes, "scales": scales, "format": FORMAT,
            "shape": torch.tensor([int(codes.shape[0]), int(codes.shape[1]) * 2], dtype=torch.int64)}


def _parts(q, result: dict):
    """(codes, scales, N, K) of a result, on the compute device, shapes checked."""
    if result.get("format") != FORMAT:
        raise ValueError(f"not an mxfp4 result (format {result.get('format')!r})")
    N, K = (int(v) for v in result["shape"].tolist())
    dev = q.compute_device()
    codes = result["codes"].to(dev).contiguous()
    scales = result["scales"].to(dev).contiguous()
    if K % BLOCK != 0 or tuple(codes.shape) != (N, K // 2) or tuple(scales.shape) != (N, K // BLOCK):
        raise ValueError(f"mxfp4 result: codes {tuple(codes.shape)} / scales {tuple(scales.shape)} do not match "
                         f"shape [{N}, {K}]")
    return codes, scales, N, K


def dequantize_mxfp4(q, result: dict, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The weight an MXFP4 result stands for, [N, K] of `dtype` (bf16 / fp16 / fp32) on the compute
    device: +-mag 2^(e - 127), rounded once; a block whose scale byte is 255 is NaN."""
    if dtype not in DTYPES:
        raise ValueError(f"dequantize_mxfp4 writes bf16 / fp16 / fp32, got {dtype}")
    codes, scales, N, K = _parts(q, result)
    out = torch.empty((N, K), dtype=dtype, device=codes.device)
    _hip.dequantize_mxfp4(codes, scales, out)
    return out


def mxfp4_matmul(q, a_result: dict, w_result: dict, bias=None, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """a [T, K] times w [N, K] transposed, both MXFP4 results, (+ bias [N]) -> [T, N] of `dtype` on the
    compute device, through awq_mxfp4_gemm (both operands FP4 on the scaled matrix instruction, fp32
    accumulation, one rounding)."""
    if dtype not in DTYPES:
        raise ValueError(f"mxfp4_matmul writes bf16 / fp16 / fp32, got {dtype}")
    a_codes, a_scales, T, K = _parts(q, a_result)
    w_codes, w_scales, N, Kw = _parts(q, w_result)
    if K != Kw:
        raise ValueError(f"mxfp4_matmul: a is [{T}, {K}], w is [{N}, {Kw}]: the inner sizes differ")
    if bias is not None:
        if bias.dtype not in DTYPES or tuple(bias.shape) != (N,):
            raise ValueError(f"mxfp4_matmul: bias must be a bf16 / fp16 / fp32 [{N}], got {bias.dtype} "
                             f"{tuple(bias.shape)}")
        bias = bias.to(a_codes.device).contiguous()
    out = torch.empty((T, N), dtype=dtype, device=a_codes.device)
    _hip.mxfp4_gemm(a_codes, a_scales, w_codes, w_scales, out, bias)
    return out


def mxfp4_linear(q, x: torch.Tensor, w_result: dict, bias=None, act_rule: str = "floor", dtype=None) -> torch.Tensor:
    """F.linear with both operands in MXFP4 (W4A4): x [T, K] is block-quantized along K under `act_rule`
    (awq_quantize_mxfp4), then mxfp4_matmul with the weight result.  The output dtype defaults to x's."""
    return mxfp4_matmul(q, quantize_mxfp4(q, x, act_rule), w_result, bias, x.dtype if dtype is None else dtype)


def quantization_error(q, tensor: torch.Tensor, result: dict, per_group: bool = False, samples=None) -> dict:
    """AWQQuantizer.quantization_error for an MXFP4 result: the keys of the integer formats' report
    without samples (error_report, plus input_scaled = False), from one pass of awq_mxfp4_error."""
    if per_group or samples is not None:
        raise ValueError("quantization_error: per_group and samples are not available for an mxfp4 result")
    check_weight(tensor)
    codes, scales, N, K = _parts(q, result)
    if tuple(tensor.shape) != (N, K):
        raise ValueError(f"quantization_error: result shape [{N}, {K}] != tensor shape {list(tensor.shape)}")
    totals = _hip.mxfp4_error(device_input(tensor, codes.device), codes, scales)
    out = error_report(tensor.numel(), totals.tolist())
    out["input_scaled"] = False
    return out
