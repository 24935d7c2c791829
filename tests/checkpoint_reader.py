"""An independent reader of the CLI's written checkpoints: an output directory -> name -> float64
weight, with plain torch integer ops on the CPU.  It calls nothing from awq_quantizer or oracle; it
is written from the layouts' descriptions (AutoAWQ's published GEMM layout, include/awq_hip.h's
wording for the packed format), so a layout slip in the kernels cannot cancel out in it.

--output_format autoawq (model.safetensors, or shards + model.safetensors.index.json), per
quantized linear `<module>`:
  qweight int32 [K, N/8]   nibble i of word c of row k = q[n = 8c + ORDER[i], k]
  qzeros  int32 [G, N/8]   the same rule, z[n, g]
  scales  fp16  [G, N]
  -> `<module>.weight` [N, K] = (q - z) * s with g = k // group_size (quant_config.json)
ORDER = 0, 2, 4, 6, 1, 3, 5, 7.  Every other tensor passes through.

--output_format packed (model_chunk_NNNN.safetensors or .pt + metadata.json), per tensor `<name>`:
  qweight int32 [rows, ceil(K * bits / 32)]   element k of a row = field k % (32 / bits) of word
                                              k // (32 / bits), low bits first, value q - qmin
  qzeros  int32 [rows, ceil(G * bits / 32)]   the same packing of the zero points
  scales  fp16  [rows, G];  bits, group_size, symmetric, shape
  -> `<name>` of `shape` = (q - z) * s; qmin = 0, or -2^(bits-1) when symmetric.

The products are formed in float64 (exact: 5 + 11 significant bits)."""
import glob
import json
import os
from typing import Dict, Tuple

import torch

ORDER = (0, 2, 4, 6, 1, 3, 5, 7)
IDENTITY = (0, 1, 2, 3, 4, 5, 6, 7)


def fields(words: torch.Tensor, bits: int = 4) -> torch.Tensor:
    """int32 [..., W] -> int64 [..., W, 32 / bits]: the fields of every word, low bits first."""
    w = words.to(torch.int64) & 0xFFFFFFFF
    shifts = torch.arange(0, 32, bits, dtype=torch.int64)
    return (w.unsqueeze(-1) >> shifts) & ((1 << bits) - 1)


def gemm_columns(words: torch.Tensor, order=ORDER) -> torch.Tensor:
    """[R, N/8] words of the GEMM layout -> int64 [R, N]: column 8c + order[i] = nibble i of word c."""
    f = fields(words, 4)                                        # [R, N/8, 8]
    out = torch.empty_like(f)
    out[..., list(order)] = f
    return out.reshape(words.shape[0], -1)


def dequant_gemm(qweight, qzeros, scales, group_size: int, order=ORDER, zero_shift: int = 0) -> torch.Tensor:
    """One GEMM-layout linear -> float64 [N, K].  order / zero_shift: what a wrong reader would do
    (the mutations of tests/test_model_forward_host.py); the defaults are the layout."""
    q = gemm_columns(qweight, order)                            # [K, N]
    z = gemm_columns(qzeros, order) + zero_shift                # [G, N]
    K = q.shape[0]
    g = torch.arange(K) // group_size
    return ((q - z[g]).double() * scales.double()[g]).t().contiguous()


def dequant_packed(r: Dict[str, torch.Tensor]) -> torch.Tensor:
    bits, L = int(r["bits"]), int(r["group_size"])
    qmin = -(1 << (bits - 1)) if bool(r["symmetric"]) else 0
    shape = [int(v) for v in r["shape"].tolist()]
    rows = shape[0] if len(shape) > 1 else 1
    K = 1
    for v in shape:
        K *= v
    K //= rows
    G = -(-K // L)
    q = fields(r["qweight"].reshape(rows, -1), bits).reshape(rows, -1)[:, :K] + qmin
    z = fields(r["qzeros"].reshape(rows, -1), bits).reshape(rows, -1)[:, :G] + qmin
    g = torch.arange(K) // L
    return ((q - z[:, g]).double() * r["scales"].reshape(rows, G).double()[:, g]).reshape(shape)


def _load_safetensors(path: str) -> Dict[str, torch.Tensor]:
    from safetensors.torch import load_file
    return load_file(path)


def read_autoawq(out_dir: str, order=ORDER, zero_shift: int = 0) -> Tuple[Dict[str, torch.Tensor], dict]:
    with open(os.path.join(out_dir, "quant_config.json")) as f:
        qcfg = json.load(f)
    L = int(qcfg["q_group_size"])
    raw: Dict[str, torch.Tensor] = {}
    index = os.path.join(out_dir, "model.safetensors.index.json")
    if os.path.isfile(index):
        with open(index) as f:
            files = sorted(set(json.load(f)["weight_map"].values()))
    else:
        files = ["model.safetensors"]
    for fn in files:
        raw.update(_load_safetensors(os.path.join(out_dir, fn)))
    state, quantized = {}, {}
    for name, t in raw.items():
        if name.endswith(".qweight"):
            mod = name[: -len(".qweight")]
            parts = (t, raw[mod + ".qzeros"], raw[mod + ".scales"])
            state[mod + ".weight"] = dequant_gemm(*parts, L, order, zero_shift)
            quantized[mod + ".weight"] = dict(zip(("qweight", "qzeros", "scales"), parts))
        elif name.endswith((".qzeros", ".scales")) and name.rsplit(".", 1)[0] + ".qweight" in raw:
            continue
        else:
            state[name] = t.double()
    return state, {"format": "autoawq", "group_size": L, "quantized": quantized, "quant_config": qcfg}


def read_packed(out_dir: str) -> Tuple[Dict[str, torch.Tensor], dict]:
    with open(os.path.join(out_dir, "metadata.json")) as f:
        meta = json.load(f)
    results: Dict[str, Dict[str, torch.Tensor]] = {}
    for path in sorted(glob.glob(os.path.join(out_dir, "model_chunk_*"))):
        if path.endswith(".safetensors"):
            for key, t in _load_safetensors(path).items():
                name, field = key.rsplit(".", 1)
                results.setdefault(name, {})[field] = t
        else:
            results.update(torch.load(path, map_location="cpu", weights_only=True))
    assert set(results) == set(meta["tensor_to_chunk"]), "metadata.json does not list the chunks' tensors"
    state = {name: dequant_packed(r) for name, r in results.items()}
    return state, {"format": "packed", "quantized": results}


def read_checkpoint(out_dir: str) -> Tuple[Dict[str, torch.Tensor], dict]:
    """(name -> float64 tensor, info) of an --output_format autoawq or packed directory."""
    if os.path.isfile(os.path.join(out_dir, "quant_config.json")):
        return read_autoawq(out_dir)
    return read_packed(out_dir)
