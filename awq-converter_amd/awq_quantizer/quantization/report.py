"""The quantization-error report (include/awq_hip.h awq_quant_error / awq_output_error) behind
AWQQuantizer.quantization_error / quantization_error_model, whose docstrings say what goes in and
what comes out, and the figures derived from the kernels' sums (error_report, output_report).
"""
import math
from typing import Dict, Optional

import torch

from .. import _hip
from ..layout import aligned, device_input, packed_shapes, read_meta


def quantization_error(q, tensor: torch.Tensor, result: Dict[str, torch.Tensor], per_group: bool = False,
                       samples: Optional[torch.Tensor] = None) -> dict:
    """What `result` costs against the original `tensor`, in weight space and on `samples`."""
    q._check_input(tensor)
    if tensor.dtype == torch.float64:
        raise RuntimeError("quantization_error: float64 weights are not supported")
    bits, L, sym = read_meta(result, "bits", "group_size", "symmetric")
    scales = result["scales"]
    if scales.dim() != 2:
        raise IndexError(f"too many indices for tensor of dimension {scales.dim()}")
    n = tensor.numel()
    sh = packed_shapes(tensor.shape, L, bits)
    rows, K, G = sh["rows"], sh["K"], sh["G"]
    if tuple(scales.shape) != (rows, G):
        raise IndexError(f"scales shape {tuple(scales.shape)} does not match {rows} rows x {G} groups")
    in_scale = result.get("input_scale")
    if in_scale is not None and (tensor.dim() != 2 or tuple(in_scale.shape) != (K,)):
        raise ValueError(f"quantization_error: input_scale {tuple(in_scale.shape)} does not match a 2-D weight "
                         f"[out, {K}] (tensor shape {tuple(tensor.shape)})")
    if samples is not None and (tensor.dim() != 2 or samples.dim() != 2 or samples.shape[1] != K):
        raise ValueError(f"quantization_error: samples {tuple(samples.shape)} do not match a 2-D weight "
                         f"[out, {K}] (tensor shape {tuple(tensor.shape)})")
    dev = q.compute_device()
    w = w_orig = device_input(tensor, dev)
    if in_scale is not None:     # the result quantizes W * diag(input_scale): measure against that
        w = _hip.apply_input_scale(w, in_scale.to(dev, torch.float32).contiguous())
    scales = scales.to(dev, torch.float16).contiguous()
    if "qweight" in result:
        if "shape" in result and read_meta(result, "shape")[0] != tuple(tensor.shape):
            raise ValueError(f"quantization_error: result shape {result['shape'].tolist()} != tensor shape "
                             f"{list(tensor.shape)}")
        qweight = result["qweight"].to(dev, torch.int32).contiguous()
        qzeros = result["qzeros"].to(dev, torch.int32).contiguous()
    else:
        tq, zp = result["tensor_q"], result["zero_points"]
        if tuple(tq.shape) != tuple(tensor.shape) or tuple(zp.shape) != (rows, G):
            raise ValueError(f"quantization_error: tensor_q {tuple(tq.shape)} / zero_points {tuple(zp.shape)} "
                             f"do not match tensor shape {tuple(tensor.shape)}")
        qmin = -(1 << (bits - 1)) if sym else 0
        qweight = torch.empty(sh["qweight"], dtype=torch.int32, device=dev)
        qzeros = torch.empty(sh["qzeros"], dtype=torch.int32, device=dev)
        if n:
            _hip.pack_rows(tq.to(dev, torch.int32).contiguous(), rows, K, bits, qmin, qweight)
            _hip.pack_rows(zp.to(dev, torch.int32).contiguous(), rows, G, bits, qmin, qzeros)
    if tuple(qweight.shape) != sh["qweight"] or tuple(qzeros.shape) != sh["qzeros"]:
        raise ValueError(f"quantization_error: qweight {tuple(qweight.shape)} / qzeros {tuple(qzeros.shape)} "
                         f"do not match tensor shape {tuple(tensor.shape)}")
    stats, bad, totals = _hip.quant_error(w, rows, K, L, bits, sym, aligned(qweight), qzeros, scales)
    out = error_report(n, totals.tolist())
    out["input_scaled"] = in_scale is not None
    if samples is not None:
        col = in_scale.to(dev, torch.float32).contiguous() if in_scale is not None else None
        e_sq, r_sq, _ = _hip.output_error(w_orig, L, bits, sym, aligned(qweight), qzeros, scales,
                                          device_input(samples.to(w_orig.dtype), dev), col)
        out.update(output_report(float(e_sq.double().sum()), float(r_sq.double().sum()), samples.shape[0]))
        if per_group:
            out.update(row_output_sq=e_sq, row_output_ref_sq=r_sq)
    if per_group:
        out.update(group_abs=stats[0].view(rows, G), group_sq=stats[1].view(rows, G),
                   group_w_sq=stats[2].view(rows, G), group_max=stats[3].view(rows, G),
                   group_nonfinite=bad.view(rows, G))
    return out


def quantization_error_model(q, tensors: Dict[str, torch.Tensor],
                             results: Dict[str, Dict[str, torch.Tensor]]) -> Dict[str, dict]:
    """quantization_error for every result; failures are logged and skipped."""
    out = {}
    for name, res in results.items():
        try:
            if name not in tensors:
                raise KeyError(f"no source tensor named {name}")
            out[name] = q.quantization_error(tensors[name], res)
        except Exception as e:  # skip and continue
            q.logger.error(f"Error measuring tensor: {name}, error: {e}")
            continue
    return out

def output_report(err_sq: float, ref_sq: float, tokens: int) -> dict:
    """The output-space figures from the sums of awq_output_error's err_sq / ref_sq over a tensor's
    rows — or over a model: the sums add."""
    if err_sq == 0.0:
        snr = math.inf
    elif err_sq != err_sq or ref_sq != ref_sq:
        snr = math.nan
    else:
        snr = 10.0 * math.log10(ref_sq / err_sq) if ref_sq > 0.0 else -math.inf
    rel = math.sqrt(err_sq / ref_sq) if ref_sq > 0.0 and err_sq >= 0.0 else (0.0 if err_sq == 0.0 else math.nan)
    return {"output_sum_sq": err_sq, "output_ref_sq": ref_sq, "output_rel_error": rel, "output_snr_db": snr,
            "output_tokens": int(tokens)}


def error_report(numel: int, totals) -> dict:
    """The report's numbers from awq_quant_error's totals (sum |d|, sum d^2, sum w^2, max |d|,
    non-finite count) of a tensor — or of a model: the sums and counts add, the max is the max."""
    sum_abs, sum_sq, sum_w_sq, max_abs, bad = (float(v) for v in totals)
    finite = int(numel) - int(bad)
    if sum_sq == 0.0:
        snr = math.inf
    else:
        snr = 10.0 * math.log10(sum_w_sq / sum_sq) if sum_w_sq > 0.0 else -math.inf
    return {"numel": int(numel), "nonfinite": int(bad), "sum_abs": sum_abs, "sum_sq": sum_sq, "sum_w_sq": sum_w_sq,
            "mean_abs_error": sum_abs / finite if finite else math.nan,
            "mse": sum_sq / finite if finite else math.nan,
            "max_abs_error": max_abs, "snr_db": snr}
