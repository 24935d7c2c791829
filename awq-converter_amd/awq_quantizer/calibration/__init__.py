"""Calibration pass: token ids + model directory -> the activation statistics --act_stats reads.

  calibrate_model(model_dir, input_ids)  ->  {weight name: (x_mean, x_sq)}   (main.load_act_stats' shape)
  save_act_stats(stats, path)            the file --act_stats / load_act_stats read
  read_input_ids(path) / chunk_text(...) the CLI's two sources of ids (awq_quantizer/calibrate.py)

The forward (forward.py) runs on the GPU through the fused HIP kernels; there is no CPU fallback
(_hip.HipUnavailable).  `ops` exists for host tests, which inject torch compositions.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import torch

from .forward import (BLOCK_LINEARS, CalibrationConfigError, DecoderConfig, HipOps, parse_config, plan_micro_batches,
                      read_config, rope_inv_freq, run_decoder, sample_rows)
from .stats import StatsAccumulator

__all__ = ["StatsAccumulator", "CalibrationConfigError", "DecoderConfig", "HipOps", "calibrate_model", "chunk_text",
           "parse_config", "plan_micro_batches", "read_config", "read_input_ids", "rope_inv_freq", "run_decoder",
           "save_act_stats", "sample_rows", "save_act_samples", "load_act_samples"]

_DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32,
           "float64": torch.float64}


def check_input_ids(ids) -> torch.Tensor:
    if not isinstance(ids, torch.Tensor):
        ids = torch.as_tensor(ids)
    if ids.dim() != 2 or ids.shape[0] == 0 or ids.shape[1] == 0:
        raise ValueError(f"input_ids must be a non-empty [n, seq] matrix, got shape {tuple(ids.shape)}")
    if ids.dtype != torch.int64:
        raise ValueError(f"input_ids must be int64, got {ids.dtype}")
    if int(ids.min()) < 0:
        raise ValueError("input_ids must be non-negative")
    return ids.contiguous()


def read_input_ids(path: str) -> torch.Tensor:
    """A safetensors file with `input_ids` int64 [n, seq], or a .npy of the same."""
    if path.endswith(".npy"):
        import numpy as np
        return check_input_ids(torch.from_numpy(np.load(path, allow_pickle=False)))
    from safetensors.torch import load_file
    flat = load_file(path)
    if "input_ids" not in flat:
        raise ValueError(f"{path} has no tensor named input_ids")
    return check_input_ids(flat["input_ids"])


def chunk_text(text: str, tokenizer, seq_len: int, n_samples: int) -> torch.Tensor:
    """The text tokenised (tokenizers.Tokenizer), its ids cut into seq_len blocks, the first n_samples kept."""
    ids = tokenizer.encode(text).ids
    n = min(len(ids) // seq_len, n_samples)
    if n == 0:
        raise ValueError(f"the text gives {len(ids)} tokens: not one block of seq_len {seq_len}")
    return torch.tensor(ids[:n * seq_len], dtype=torch.int64).view(n, seq_len)


def resolve_dtype(compute_dtype, checkpoint_dtype: Optional[torch.dtype]) -> torch.dtype:
    if compute_dtype is None:
        compute_dtype = checkpoint_dtype
    if isinstance(compute_dtype, str):
        if compute_dtype not in _DTYPES:
            raise ValueError(f"compute_dtype: one of {', '.join(_DTYPES)}, got {compute_dtype!r}")
        compute_dtype = _DTYPES[compute_dtype]
    if compute_dtype not in _DTYPES.values():
        raise ValueError(f"compute_dtype {compute_dtype} is not a floating-point dtype the forward runs in")
    return compute_dtype


def calibrate_model(model_dir: str, input_ids, compute_dtype=None, batch_tokens: int = 8192, device="cuda",
                    ops=None, logger=None, n_sample_tokens: int = 0,
                    samples_out: Optional[Dict[str, torch.Tensor]] = None
                    ) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """Statistics of every linear's input over input_ids [n, seq]: weight name -> (x_mean, x_sq), fp32
    [in_features] on the CPU.  compute_dtype: the checkpoint's dtype by default; float32 is allowed
    (float64 only with injected ops: the kernels take bf16 / fp16 / fp32).  n_sample_tokens > 0
    with a dict samples_out: run_decoder's token samples, "<block>.<group>.samples" -> [n, in]."""
    from ..model_loading.safetensors_loader import SafetensorsLoader
    ids = check_input_ids(input_ids)
    if batch_tokens <= 0:
        raise ValueError("batch_tokens must be positive")
    cfg = parse_config(read_config(model_dir), seq_len=ids.shape[1], max_id=int(ids.max()))   # before the model is read
    device = torch.device(device)
    if ops is None:
        ops = HipOps(device)
    loader = SafetensorsLoader(model_dir, logger_level="WARNING")
    try:
        index = {i.name: i for i in loader.tensor_index()}
        embed = index.get("model.embed_tokens.weight") or index.get("embed_tokens.weight")
        dtype = resolve_dtype(compute_dtype, embed.dtype if embed is not None else None)
        if isinstance(ops, HipOps) and dtype == torch.float64:
            raise ValueError("compute_dtype float64: the calibration kernels take bfloat16 / float16 / float32")
        return run_decoder(loader, cfg, ids, dtype, device, ops, batch_tokens=batch_tokens, logger=logger,
                           n_sample_tokens=n_sample_tokens, samples_out=samples_out)
    finally:
        loader.close()


def save_act_stats(stats: Dict[str, Tuple[torch.Tensor, torch.Tensor]], path: str) -> None:
    from safetensors.torch import save_file
    flat = {}
    for name, (m, s) in stats.items():
        flat[name + ".x_mean"] = m.detach().float().cpu().contiguous().clone()
        flat[name + ".x_sq"] = s.detach().float().cpu().contiguous().clone()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    save_file(flat, path, metadata={"format": "pt"})


def save_act_samples(samples: Dict[str, torch.Tensor], path: str) -> None:
    """The token samples of a calibration pass ("<block>.<group>.samples" -> [tokens, in]) as their
    own safetensors file: the statistics file keeps exactly its keys."""
    from safetensors.torch import save_file
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    save_file({k: v.detach().cpu().contiguous().clone() for k, v in samples.items()}, path, metadata={"format": "pt"})


def group_samples(flat: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """"<block>.<group>.samples" tensors -> weight name -> its group's tensor (BLOCK_LINEARS)."""
    out = {}
    for key, t in flat.items():
        if not key.endswith(".samples"):
            continue
        block, _, group = key[: -len(".samples")].rpartition(".")
        for name, mods in BLOCK_LINEARS:
            if name == group:
                for m in mods:
                    out[f"{block}.{m}.weight"] = t
    return out


def load_act_samples(path: str) -> Dict[str, torch.Tensor]:
    """A --samples_output file -> weight name -> token samples [tokens, in_features] of its input
    (the members of a group share one tensor)."""
    from safetensors.torch import load_file
    return group_samples(load_file(path))
