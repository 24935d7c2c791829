"""AutoGPTQ-layout linears (4 bits) in and out (include/awq_hip.h awq_export_gptq / awq_import_gptq;
act-order, desc_act = true: awq_gptq_permute_rows / awq_gptq_gidx_from_perm / awq_dequantize_gptq,
DESIGN.md §5.20), behind AWQQuantizer's methods of the same names: their docstrings say what each
takes and returns.

A result dict that carries "perm" (int32 [K]: perm[i] = the original input column at position i)
holds its packed tensors in permuted column order: quantize_gptq(act_order=True) and import_gptq
of a balanced act-order g_idx return such dicts, and export_gptq writes them in the act-order
layout.
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


def device_perm(perm: torch.Tensor, K: int, dev: torch.device) -> torch.Tensor:
    """`perm` as a contiguous int32 [K] on dev; ValueError unless it is a permutation of 0 .. K - 1
    (the kernels clamp what is out of range: a wrong perm would give a wrong checkpoint quietly)."""
    p = perm.detach().to(dev, torch.int32).contiguous().reshape(-1)
    if p.numel() != K or int(_hip.gptq_check_index(p, K)) != 0 or \
            not torch.equal(torch.sort(p).values, torch.arange(K, dtype=torch.int32, device=dev)):
        raise ValueError(f"perm is not a permutation of the {K} input columns")
    return p


def export_gptq(q, packed: Dict[str, torch.Tensor], checkpoint_format: str = "gptq") -> Dict[str, torch.Tensor]:
    """A quantize_packed() result of a 2-D weight in the GPTQ layout; with "perm", the act-order one."""
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
    if packed.get("perm") is None:
        _hip.export_gptq(packed["qweight"].contiguous(), qz, packed["scales"].contiguous(), N, K, L, bits, sym, off,
                         out["qweight"], out["qzeros"], out["scales"], out["g_idx"])
    else:
        # the fields leave the transpose in permuted order; the nibble-row gather puts column perm[i]'s
        # row, now at i, back at perm[i], and g_idx says which group it was rounded in
        perm = device_perm(packed["perm"], K, dev)
        tmp, invperm = torch.empty_like(out["qweight"]), torch.empty_like(perm)
        _hip.export_gptq(packed["qweight"].contiguous(), qz, packed["scales"].contiguous(), N, K, L, bits, sym, off,
                         tmp, out["qzeros"], out["scales"], None)
        _hip.gptq_gidx_from_perm(perm, L, out["g_idx"], invperm)
        _hip.gptq_permute_rows(tmp, invperm, out["qweight"])
    # v1 stores a zero point of 0 as 15, and loaders differ on masking after they add 1
    out["zero_points_at_0"] = count_zero_fields(qz, sh["G"]) if off else torch.zeros((), dtype=torch.int64, device=dev)
    return out


def act_order_perm(g: torch.Tensor, K: int, L: int) -> Optional[torch.Tensor]:
    """g_idx (int64 [K], CPU) -> the order its columns were rounded in, int64 [K]: the stable
    ascending argsort, when every one of the K / L groups has exactly L entries; None otherwise."""
    G = K // L
    if g.numel() != K or int(g.min()) < 0 or int(g.max()) >= G or not bool((torch.bincount(g, minlength=G) == L).all()):
        return None
    return torch.sort(g, stable=True).indices


def _checked(q, gptq, group_size, symmetric, checkpoint_format, any_g_idx: bool):
    """import_gptq's argument checks, all before any device work.  -> (zero_offset, group size,
    symmetric, N, K, g_idx on the CPU as int64 or None when it is absent or k // group_size)."""
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
    g = None
    if "g_idx" in gptq and gptq["g_idx"] is not None:
        g = gptq["g_idx"].to("cpu", torch.int64).reshape(-1)
        if g.numel() == K and torch.equal(g, torch.arange(K, dtype=torch.int64) // L):
            g = None
        elif any_g_idx:
            if g.numel() != K or int(g.min()) < 0 or int(g.max()) >= K // L:
                raise ValueError(f"dequantize_gptq: g_idx must hold {K} group indices in [0, {K // L})")
        elif act_order_perm(g, K, L) is None:
            raise ValueError("import_gptq: g_idx is not k // group_size (act-order, desc_act = true, is not supported)")
    return off, L, sym, N, K, g


def _on_device(gptq, dev):
    return {k: gptq[k].to(dev, torch.float16 if k == "scales" else torch.int32).contiguous()
            for k in ("qweight", "qzeros", "scales")}


def import_gptq(q, gptq: Dict[str, torch.Tensor], group_size: Optional[int] = None,
                symmetric: Optional[bool] = None, checkpoint_format: str = "gptq") -> Dict[str, torch.Tensor]:
    """A GPTQ-layout linear as a quantize_packed()-shaped dict on the device; a balanced act-order
    g_idx gives the dict in permuted column order, with "perm"."""
    off, L, sym, N, K, g = _checked(q, gptq, group_size, symmetric, checkpoint_format, False)
    dev = q.compute_device()
    src = _on_device(gptq, dev)
    perm = None
    if g is not None:
        perm = act_order_perm(g, K, L).to(dev, torch.int32)
        ordered = torch.empty_like(src["qweight"])
        _hip.gptq_permute_rows(src["qweight"], perm, ordered)
        src["qweight"] = ordered
    sh = packed_shapes((N, K), L, 4)
    out = {"qweight": torch.empty(sh["qweight"], dtype=torch.int32, device=dev),
           "qzeros": torch.empty(sh["qzeros"], dtype=torch.int32, device=dev),
           "scales": torch.empty(sh["scales"], dtype=torch.float16, device=dev)}
    _hip.import_gptq(src["qweight"], src["qzeros"], src["scales"], N, K, L, 4, sym, off, out["qweight"],
                     out["qzeros"], out["scales"])
    out.update(result_meta(4, L, sym, (N, K)))
    if perm is not None:
        out["perm"] = perm
    return out


def dequantize_gptq(q, gptq: Dict[str, torch.Tensor], group_size: Optional[int] = None,
                    symmetric: Optional[bool] = None, checkpoint_format: str = "gptq",
                    dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The [out, in] weight a GPTQ-layout linear holds: import_gptq, then dequantize_packed; with a
    g_idx that is not k // group_size (balanced or not) the fused awq_dequantize_gptq."""
    off, L, sym, N, K, g = _checked(q, gptq, group_size, symmetric, checkpoint_format, True)
    if g is None:
        return q.dequantize_packed(q.import_gptq(gptq, group_size, symmetric, checkpoint_format), dtype)
    dev = q.compute_device()
    src = _on_device(gptq, dev)
    direct = dtype in (torch.float32, torch.float16, torch.bfloat16)
    out = torch.empty((N, K), dtype=dtype if direct else torch.float32, device=dev)
    _hip.dequantize_gptq(src["qweight"], src["qzeros"], src["scales"], g.to(dev, torch.int32), off, out)
    return out if direct else out.to(dtype)
