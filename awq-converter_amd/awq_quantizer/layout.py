"""Shapes and metadata of a quantization result, and the memory layout the kernels ask of an
input — the one place that knows them.

A tensor is quantized as `rows` rows of `K` elements in groups of `group_size` along K
(reference awq.py:297-339: dim 0 is the row, a 0-d or 1-d tensor is one row); packed results
hold 32 // bits values per int32 word.  Plain Python and torch: stream.py plans its output
regions from these numbers before the native library is loaded, so nothing here imports it.
"""
import math
from typing import Tuple

import torch


def rows_k(shape) -> Tuple[int, int]:
    """(rows, K) of a tensor of `shape` (an empty tensor: K = 0)."""
    n = math.prod(shape) if len(shape) else 1
    rows = 1 if len(shape) <= 1 else shape[0]
    return rows, n // max(rows, 1)


def groups(K: int, group_size: int) -> int:
    """Groups per row; the tail group counts (awq.py:337-339).  No groups in an empty row."""
    return -(-K // group_size) if K else 0


def row_shapes(rows: int, K: int, group_size: int, bits: int) -> dict:
    """Shapes of the packed outputs of `rows` rows of K elements."""
    per = 32 // bits
    G = groups(K, group_size)
    return {"qweight": (rows, -(-K // per)), "qzeros": (rows, -(-G // per)), "scales": (rows, G),
            "rows": rows, "K": K, "G": G}


def packed_shapes(shape, group_size: int, bits: int) -> dict:
    """row_shapes for an input of `shape`."""
    return row_shapes(*rows_k(shape), group_size, bits)


def gptq_shapes(N: int, K: int, group_size: int) -> dict:
    """Shapes of a 4-bit GPTQ-layout linear [N = out_features, K = in_features] (include/awq_hip.h
    awq_export_gptq): packed along K in qweight, along N in qzeros."""
    G = K // group_size
    return {"qweight": (K // 8, N), "qzeros": (G, N // 8), "scales": (G, N), "g_idx": (K,), "G": G}


def result_meta(bits: int, group_size: int, symmetric: bool, shape=None) -> dict:
    """The metadata tensors of a result dict: bits / group_size (int32 0-d), symmetric (bool 0-d)
    and, for packed results, the input's shape (int64)."""
    meta = {"bits": torch.tensor(bits, dtype=torch.int32),
            "group_size": torch.tensor(group_size, dtype=torch.int32),
            "symmetric": torch.tensor(symmetric, dtype=torch.bool)}
    if shape is not None:
        meta["shape"] = torch.tensor(list(shape), dtype=torch.int64)
    return meta


_READ = {"bits": int, "group_size": int, "symmetric": bool}


def read_meta(result: dict, *keys: str) -> tuple:
    """The named metadata of a result dict as Python values, in the order asked for
    ("shape": a tuple of ints).  A missing key is the dict's KeyError."""
    return tuple(tuple(int(v) for v in result[k].tolist()) if k == "shape" else _READ[k](result[k].item())
                 for k in keys)


def aligned(x: torch.Tensor) -> torch.Tensor:
    """The streaming kernel's 16-B vector loads need a 16-B aligned base: a misaligned
    device view (e.g. flat[4:4100]) is copied into fresh (aligned) storage."""
    return x if x.data_ptr() % 16 == 0 else x.clone()


def device_input(v: torch.Tensor, dev: torch.device) -> torch.Tensor:
    if v.device == dev and v.is_contiguous():
        return aligned(v)
    return v.detach().to(dev).contiguous()
