"""AutoGPTQ-layout linears (4 bits, desc_act = false) in and out (include/awq_hip.h awq_export_gptq /
awq_import_gptq), behind AWQQuantizer's methods of the same names: their docstrings say what each
takes and returns.
"""
from typing import Dict, Optional

import torch

from .. import _hip
from ..layout import gptq_shapes, packed_shapes, read_meta, result_meta

# checkpoint_format -> zero_offset: what a loader adds to a stored zero ("gptq", v1, stores z - 1)
CHECKPOINT_FORMATS = {"gptq": 1, "gptq_v2": 0}


def zero_offset_of(checkpoint_format: str) -> int:
    if checkpoint_format not in CHECKPOINT_FORMATS:
        raise ValueError(f"checkpoint_format must be one of {', '.join(CHECKPOINT_FORMATS)}; got {checkpoint_format!r}")
    return CHECKPOINT_FORMATS[checkpoint_format]


def count_zero_fields(qzeros: torch.Tensor, G: int) -> torch.Tensor:
    """Zero-point fields equal to 0 among the G groups of every row of a row-major packed qzeros
    [N, ceil(G/8)], as a 0-d int64 tensor on its device (no sync): under checkpoint_format "gptq"
    each is stored as 15."""
    z = qzeros.to(torch.int64) & 0xFFFFFFFF
    fields = torch.stack([(z >> (4 * i)) & 15 for i in range(8)], dim=-1).reshape(z.shape[0], -1)[:, :G]
    return (fields == 0).sum()


def export_gptq(q, packed: Dict[str, torch.Tensor], checkpoint_format: str = "gptq") -> Dict[str, torch.Tensor]:
    """A quantize_packed() result of a 2-D weight in the GPTQ layout."""
    off = zero_offset_of(checkpoint_format)
    shape, = read_meta(packed, "shape")
    if len(shape) != 2:
        raise ValueError(f"GPTQ layout is for 2-D linear weights, got shape {shape}")
    N, K = shape
    L, bits, sym = read_meta(packed, "group_size", "bits", "symmetric")
    dev = packed["qweight"].device
    sh = gptq_shapes(N, K, L)
    out = {"qweight": torch.empty(sh["qweight"], dtype=torch.int32, device=dev),
           "qzeros": torch.empty(sh["qzeros"], dtype=torch.int32, device=dev),
           "scales": torch.empty(sh["scales"], dtype=torch.float16, device=dev),
           "g_idx": torch.empty(sh["g_idx"], dtype=torch.int32, device=dev)}
    qz = packed["qzeros"].contiguous()
    _hip.export_gptq(packed["qweight"].contiguous(), qz, packed["scales"].contiguous(), N, K, L, bits, sym, off,
                     out["qweight"], out["qzeros"], out["scales"], out["g_idx"])
    # v1 stores a zero point of 0 as 15, and loaders differ on masking after they add 1
    out["zero_points_at_0"] = count_zero_fields(qz, sh["G"]) if off else torch.zeros((), dtype=torch.int64, device=dev)
    return out


def import_gptq(q, gptq: Dict[str, torch.Tensor], group_size: Optional[int] = None,
                symmetric: Optional[bool] = None, checkpoint_format: str = "gptq") -> Dict[str, torch.Tensor]:
    """A GPTQ-layout linear as a quantize_packed()-shaped dict on the device."""
    off = zero_offset_of(checkpoint_format)
    L = q.group_size if group_size is None else int(group_size)
    sym = q.symmetric if symmetric is None else bool(symmetric)
    for k in ("qweight", "qzeros", "scales"):
        if k not in gptq or gptq[k].dim() != 2:
            raise ValueError(f"import_gptq: '{k}' must be a 2-D tensor of the GPTQ layout")
    K, N = int(gptq["qweight"].shape[0]) * 8, int(gptq["qweight"].shape[1])
    if L <= 0 or K % L != 0:
        raise ValueError(f"import_gptq: in_features {K} is not a multiple of group_size {L}")
    if N % 8 != 0:
        raise ValueError(f"import_gptq: out_features {N} is not a multiple of 8")
    want = gptq_shapes(N, K, L)
    for k in ("qweight", "qzeros", "scales"):
        if tuple(gptq[k].shape) != want[k]:
            raise ValueError(f"import_gptq: {k} shape {tuple(gptq[k].shape)} != {want[k]} "
                             f"(qweight [K/8, N], qzeros [K/gs, N/8], scales [K/gs, N]; group_size {L})")
    if "g_idx" in gptq and gptq["g_idx"] is not None:
        g = gptq["g_idx"].to("cpu", torch.int64).reshape(-1)
        if g.numel() != K or not torch.equal(g, torch.arange(K, dtype=torch.int64) // L):
            raise ValueError("import_gptq: g_idx is not k // group_size (act-order, desc_act = true, is not supported)")
    dev = q.compute_device()
    src = {k: gptq[k].to(dev, torch.float16 if k == "scales" else torch.int32).contiguous()
           for k in ("qweight", "qzeros", "scales")}
    sh = packed_shapes((N, K), L, 4)
    out = {"qweight": torch.empty(sh["qweight"], dtype=torch.int32, device=dev),
           "qzeros": torch.empty(sh["qzeros"], dtype=torch.int32, device=dev),
           "scales": torch.empty(sh["scales"], dtype=torch.float16, device=dev)}
    _hip.import_gptq(src["qweight"], src["qzeros"], src["scales"], N, K, L, 4, sym, off, out["qweight"],
                     out["qzeros"], out["scales"])
    out.update(result_meta(4, L, sym, (N, K)))
    return out


def dequantize_gptq(q, gptq: Dict[str, torch.Tensor], group_size: Optional[int] = None,
                    symmetric: Optional[bool] = None, checkpoint_format: str = "gptq",
                    dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """import_gptq, then dequantize_packed: the [out, in] weight a GPTQ-layout linear holds."""
    return q.dequantize_packed(q.import_gptq(gptq, group_size, symmetric, checkpoint_format), dtype)
