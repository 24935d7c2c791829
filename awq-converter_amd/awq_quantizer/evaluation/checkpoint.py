"""A written checkpoint as a loader: SafetensorsLoader's tensor_index() / read() over an output
directory of main, in every format verify reads, so the decoder forward (calibration/forward.py)
runs the quantized model exactly as it runs the source.

  reference / packed (metadata.json + model_chunk_NNNN.safetensors or .pt): every tensor the chunks
      hold is dequantized by `dequant`; a result that carries `input_scale` (--scale_method awq
      without a folded producer) is brought back to the source's domain, w^ = RN(dq / input_scale);
  autoawq (model.safetensors or its shards + quant_config.json): every qweight / qzeros / scales
      triple is dequantized, every other tensor is read as written.  A --fold_scales directory is
      used as it stands: folded norms, biases and rows with scaled-domain weights;
  gptq (the same files + quantize_config.json with quant_method "gptq"): the same, every linear
      imported through awq_import_gptq (g_idx is checked to be k // group_size and not read again).

Tensors the directory does not hold come from the source.  `dequant` does the arithmetic:
DeviceDequant runs the library's kernels (awq_dequantize, awq_dequantize_packed,
awq_import_autoawq_gemm, awq_import_gptq); host tests inject a stub.
"""
from __future__ import annotations

import json
import os
import threading
from typing import Dict, List

import torch

from ..verify import (CHUNK_STEM, _split_flat, autoawq_files, is_autoawq_dir, is_gptq_dir, read_gptq_config,
                      read_quant_config)

_GEMM_KEYS = ("qweight", "qzeros", "scales")


class DeviceDequant:
    """The three formats' dequantization on the device, through AWQQuantizer's existing entries."""

    def __init__(self, device):
        from ..quantization.awq import AWQQuantizer
        self.q = AWQQuantizer(device=str(device), logger_name="awq_evaluate_quantizer", logger_level="WARNING")
        self.device = self.q.compute_device()

    def reference(self, res: Dict[str, torch.Tensor]) -> torch.Tensor:
        try:
            return self.q.dequantize(res).to(self.device)
        except IndexError:      # a small-tensor result (0-d / 1-d scales): the same fp16 arithmetic, per tensor
            d = (res["tensor_q"].to(self.device, torch.float32) - res["zero_points"].to(self.device, torch.float32))
            return (d.half() * res["scales"].to(self.device, torch.float16)).float()

    def packed(self, res: Dict[str, torch.Tensor]) -> torch.Tensor:
        on = {k: (v.to(self.device).contiguous() if k in _GEMM_KEYS else v) for k, v in res.items()}
        return self.q.dequantize_packed(on)

    def autoawq(self, gemm: Dict[str, torch.Tensor], group_size: int, symmetric: bool) -> torch.Tensor:
        return self.q.dequantize_autoawq(gemm, group_size=group_size, symmetric=symmetric)

    def gptq(self, gptq: Dict[str, torch.Tensor], group_size: int, symmetric: bool,
             checkpoint_format: str) -> torch.Tensor:
        return self.q.dequantize_gptq(gptq, group_size=group_size, symmetric=symmetric,
                                      checkpoint_format=checkpoint_format)

    def unscale(self, w: torch.Tensor, input_scale: torch.Tensor) -> torch.Tensor:
        return w.float() / input_scale.to(w.device, torch.float32)[None, :]


class QuantizedCheckpoint:
    """tensor_index() / read() over `quantized_dir`, backed by the source loader."""

    def __init__(self, source, quantized_dir: str, dequant):
        self.source, self.dir, self.dequant = source, quantized_dir, dequant
        self.model_path = getattr(source, "model_path", None)
        self._src = {i.name: i for i in source.tensor_index()}
        self._cache = (None, None)            # (chunk number, its results): one chunk resident
        self._handles: List[object] = []
        self._lock = threading.Lock()         # run_decoder reads the next block ahead on a worker thread
        if is_autoawq_dir(quantized_dir):
            from safetensors import safe_open
            self.format = "gptq" if is_gptq_dir(quantized_dir) else "autoawq"
            read = read_gptq_config if self.format == "gptq" else read_quant_config
            cfg, problems = read(quantized_dir)
            if problems:
                raise ValueError("; ".join(f"{k}: {v}" for k, v in problems.items()))
            self._gs, self._sym = cfg["group_size"], cfg["symmetric"]
            self._ckpt_format = cfg.get("checkpoint_format")
            self._where: Dict[str, object] = {}
            for shard in autoawq_files(quantized_dir):
                h = safe_open(shard, framework="pt")
                self._handles.append(h)
                for k in h.keys():
                    self._where[k] = h
        else:
            meta_path = os.path.join(quantized_dir, "metadata.json")
            if not os.path.exists(meta_path):
                raise FileNotFoundError(f"{quantized_dir} holds neither metadata.json nor model.safetensors: not a "
                                        f"directory main wrote")
            with open(meta_path) as f:
                self._meta = json.load(f)
            self.format = "chunks"
            self._chunk_of = {k: int(v) for k, v in self._meta["tensor_to_chunk"].items()}
        unknown = [n for n in self.quantized_names() if n not in self._src]
        if unknown:
            raise ValueError(f"{quantized_dir}: {unknown[0]} has no source tensor of this name")

    def quantized_names(self) -> List[str]:
        """The tensors that are dequantized from the directory (source names)."""
        if self.format == "chunks":
            return list(self._chunk_of)
        return sorted(n[: -len("qweight")] + "weight" for n in self._where
                      if n.endswith(".qweight") and all(n[: -len("qweight")] + k in self._where for k in _GEMM_KEYS))

    def tensor_index(self):
        return self.source.tensor_index()

    def _chunk(self, c: int) -> Dict[str, Dict[str, torch.Tensor]]:
        if self._cache[0] != c:
            st = self._meta.get("format") == "safetensors"
            path = os.path.join(self.dir, CHUNK_STEM.format(c) + (".safetensors" if st else ".pt"))
            if st:
                from safetensors.torch import load_file
                chunk = _split_flat(load_file(path))
            else:
                chunk = torch.load(path, map_location="cpu", weights_only=True)
            self._cache = (c, chunk)
        return self._cache[1]

    def read(self, info) -> torch.Tensor:
        with self._lock:
            return self._read(info)

    def _read(self, info) -> torch.Tensor:
        name = info.name
        if self.format == "chunks":
            if name not in self._chunk_of:
                return self.source.read(info)
            res = self._chunk(self._chunk_of[name])[name]
            w = self.dequant.packed(res) if "qweight" in res else self.dequant.reference(res)
            w = w.reshape(tuple(info.shape))
            if "input_scale" in res:
                w = self.dequant.unscale(w, res["input_scale"])
            return w
        layer = name[: -len(".weight")] if name.endswith(".weight") else None
        if layer is not None and all(f"{layer}.{k}" in self._where for k in _GEMM_KEYS):
            gemm = {k: self._where[f"{layer}.{k}"].get_tensor(f"{layer}.{k}") for k in _GEMM_KEYS}
            if self.format == "gptq":
                if f"{layer}.g_idx" in self._where:
                    gemm["g_idx"] = self._where[f"{layer}.g_idx"].get_tensor(f"{layer}.g_idx")
                return self.dequant.gptq(gemm, self._gs, self._sym, self._ckpt_format)
            return self.dequant.autoawq(gemm, self._gs, self._sym)
        if name in self._where:
            return self._where[name].get_tensor(name)
        return self.source.read(info)

    def close(self) -> None:
        self._handles.clear()
        self._cache = (None, None)
