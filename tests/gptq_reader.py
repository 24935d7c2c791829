"""An independent reader of --output_format gptq directories: name -> float64 weight, with plain
torch integer ops on the CPU.  It calls nothing from awq_quantizer, oracle or tests/gptq_layout.py;
it is written from AutoGPTQ's published 4-bit layout and dequantization formula, so a layout slip
in the kernels cannot cancel out in it.

Per quantized linear `<module>` [N = out_features, K = in_features], G = K / group_size:
  qweight int32 [K/8, N]   element k of output n = bits 4 (k % 8) .. of word (k // 8, n)
  qzeros  int32 [G, N/8]   zero of (group g, output n) = bits 4 (n % 8) .. of word (g, n // 8)
  scales  fp16  [G, N]
  g_idx   int32 [K]        the group of input k
  -> `<module>.weight`[n, k] = (u - ((zs + offset) & 15)) * scales[g_idx[k], n]
offset = 1 for checkpoint_format "gptq", 0 for "gptq_v2" (quantize_config.json); the mask comes
after the add.  Every other tensor passes through.  The products are formed in float64 (exact)."""
import json
import os
from typing import Dict, Tuple

import torch

OFFSET = {"gptq": 1, "gptq_v2": 0}


def dequant_gptq(qweight, qzeros, scales, g_idx, offset: int) -> torch.Tensor:
    """One GPTQ linear -> float64 [N, K]."""
    K8, N = qweight.shape
    sh = torch.arange(0, 32, 4, dtype=torch.int64)
    u = ((qweight.to(torch.int64) & 0xFFFFFFFF)[:, None, :] >> sh[None, :, None]) & 15      # [K/8, 8, N]
    u = u.reshape(K8 * 8, N)                                                                # [K, N]
    zs = ((qzeros.to(torch.int64) & 0xFFFFFFFF)[:, :, None] >> sh[None, None, :]) & 15      # [G, N/8, 8]
    z = (zs.reshape(qzeros.shape[0], N) + offset) & 15                                      # [G, N]
    g = g_idx.to(torch.int64)
    return ((u - z[g]).double() * scales.double()[g]).t().contiguous()


def read_gptq(out_dir: str) -> Tuple[Dict[str, torch.Tensor], dict]:
    from safetensors.torch import load_file
    with open(os.path.join(out_dir, "quantize_config.json")) as f:
        qcfg = json.load(f)
    offset = OFFSET[qcfg["checkpoint_format"]]
    raw = load_file(os.path.join(out_dir, "model.safetensors"))
    state, quantized = {}, {}
    parts = ("qweight", "qzeros", "scales", "g_idx")
    for name, t in raw.items():
        mod, _, field = name.rpartition(".")
        if field == "qweight":
            p = {k: raw[f"{mod}.{k}"] for k in parts}
            state[mod + ".weight"] = dequant_gptq(p["qweight"], p["qzeros"], p["scales"], p["g_idx"], offset)
            quantized[mod + ".weight"] = p
        elif field in parts and f"{mod}.qweight" in raw:
            continue
        else:
            state[name] = t.double()
    return state, {"format": "gptq", "group_size": int(qcfg["group_size"]), "quantized": quantized,
                   "quantize_config": qcfg}
