"""AutoAWQ "GEMM" checkpoints in and out, and the inverse of quantize_packed (include/awq_hip.h
awq_export_autoawq_gemm / awq_import_autoawq_gemm / awq_dequantize_packed), behind
AWQQuantizer's methods of the same names: their docstrings say what each takes and returns.
"""
from typing import Dict, Optional

import torch

from .. import _hip
from ..layout import packed_shapes, read_meta, result_meta, rows_k


def export_autoawq(q, packed: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A quantize_packed() result of a 2-D weight in the GEMM layout."""
    shape, = read_meta(packed, "shape")
    if len(shape) != 2:
        raise ValueError(f"AutoAWQ GEMM layout is for 2-D linear weights, got shape {shape}")
    N, K = shape
    L, bits = read_meta(packed, "group_size", "bits")
    dev = packed["qweight"].device
    G = K // L
    out = {"qweight": torch.empty((K, N // 8), dtype=torch.int32, device=dev),
           "qzeros": torch.empty((G, N // 8), dtype=torch.int32, device=dev),
           "scales": torch.empty((G, N), dtype=torch.float16, device=dev)}
    _hip.export_autoawq_gemm(packed["qweight"].contiguous(), packed["qzeros"].contiguous(),
                             packed["scales"].contiguous(), N, K, L, bits, out["qweight"], out["qzeros"],
                             out["scales"])
    return out


def import_autoawq(q, gemm: Dict[str, torch.Tensor], group_size: Optional[int] = None,
                   symmetric: Optional[bool] = None) -> Dict[str, torch.Tensor]:
    """A GEMM-layout linear as a quantize_packed()-shaped dict on the device."""
    L = q.group_size if group_size is None else int(group_size)
    sym = q.symmetric if symmetric is None else bool(symmetric)
    for k in ("qweight", "qzeros", "scales"):
        if k not in gemm or gemm[k].dim() != 2:
            raise ValueError(f"import_autoawq: '{k}' must be a 2-D tensor of the AutoAWQ GEMM layout")
    K, N = int(gemm["qweight"].shape[0]), int(gemm["qweight"].shape[1]) * 8
    if L <= 0 or K % L != 0:
        raise ValueError(f"import_autoawq: in_features {K} is not a multiple of group_size {L}")
    G = K // L
    want = {"qweight": (K, N // 8), "qzeros": (G, N // 8), "scales": (G, N)}
    for k, shape in want.items():
        if tuple(gemm[k].shape) != shape:
            raise ValueError(f"import_autoawq: {k} shape {tuple(gemm[k].shape)} != {shape} "
                             f"(qweight [K, N/8], qzeros [K/gs, N/8], scales [K/gs, N]; group_size {L})")
    dev = q.compute_device()
    src = {k: gemm[k].to(dev, torch.float16 if k == "scales" else torch.int32).contiguous() for k in want}
    sh = packed_shapes((N, K), L, 4)
    out = {"qweight": torch.empty(sh["qweight"], dtype=torch.int32, device=dev),
           "qzeros": torch.empty(sh["qzeros"], dtype=torch.int32, device=dev),
           "scales": torch.empty(sh["scales"], dtype=torch.float16, device=dev)}
    _hip.import_autoawq_gemm(src["qweight"], src["qzeros"], src["scales"], N, K, L, 4, out["qweight"],
                             out["qzeros"], out["scales"])
    out.update(result_meta(4, L, sym, (N, K)))
    return out


def dequantize_autoawq(q, gemm: Dict[str, torch.Tensor], group_size: Optional[int] = None,
                       symmetric: Optional[bool] = None, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """import_autoawq, then dequantize_packed: the [out, in] weight a GEMM-layout linear holds."""
    return q.dequantize_packed(q.import_autoawq(gemm, group_size, symmetric), dtype)


def dequantize_packed(q, packed: Dict[str, torch.Tensor], dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Inverse of quantize_packed with the reference's dequantize arithmetic (fp16 math)."""
    shape, L, bits, sym = read_meta(packed, "shape", "group_size", "bits", "symmetric")
    rows, K = rows_k(shape)
    out = torch.empty(shape, dtype=torch.float32, device=packed["qweight"].device)
    _hip.dequantize_packed(packed["qweight"], packed["qzeros"], packed["scales"], rows, K, L, bits, sym, out)
    return out if dtype == torch.float32 else out.to(dtype)
