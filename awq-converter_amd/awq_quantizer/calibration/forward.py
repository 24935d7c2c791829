"""Decoder forward for calibration: token ids + checkpoint -> statistics of every linear's input.

A Llama-layout decoder (model types block_plan.SUPPORTED) written against torch on the device:
embedding, RMSNorm, q / k / v (optional biases), RoPE (rotate-half), grouped-query causal
attention (scaled_dot_product_attention), o_proj, SwiGLU, down_proj, final norm.  GEMMs and
attention are torch's; the three memory-bound ops whose output a linear reads — the norm, the
SwiGLU product, and the statistics of a finished activation — are injected (`ops`), so the
product runs them as fused HIP kernels (HipOps: include/awq_hip.h awq_rmsnorm_stats,
awq_swiglu_stats, awq_act_stats_accum) and a host test can drive the same code with torch
compositions.  The pass ends at the final norm: statistics are of linear inputs, the lm_head GEMM
never runs (and without lm_head.weight in the checkpoint the final norm does not either).

One accumulator per distinct input, shared by the linears that read it:
  input_layernorm output -> q / k / v;  attention output -> o_proj;
  post_attention_layernorm output -> gate / up;  SwiGLU product -> down_proj;
  model.norm output -> lm_head (only when lm_head.weight is in the checkpoint).

The driver goes block by block: the hidden states of all samples stay resident in the compute
dtype, the block's tensors are read through SafetensorsLoader with the next block read ahead, and
the samples run in micro-batches of whole sequences of at most batch_tokens tokens — a multiple of
256 tokens wherever the sequence length allows, so that the fused kernels add to the running sums
directly (their contract: every call but the last adds whole 256-token blocks); otherwise the
producers run unfused and StatsAccumulator carries the remainders.
"""
from __future__ import annotations

import json
import math
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from ..quantization.block_plan import SUPPORTED

ROPE_TYPES = ("default", "llama3")
BLOCK_LINEARS = (("attn_in", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")),
                 ("attn_out", ("self_attn.o_proj",)),
                 ("mlp_in", ("mlp.gate_proj", "mlp.up_proj")),
                 ("mlp_out", ("mlp.down_proj",)))


class CalibrationConfigError(ValueError):
    """config.json or the ids ask for something the calibration forward does not implement."""


@dataclass
class DecoderConfig:
    model_type: str
    hidden_size: int
    num_layers: int
    num_heads: int
    num_kv_heads: int
    head_dim: int
    vocab_size: int
    max_positions: Optional[int]
    eps: float
    rope_theta: float
    rope_type: str
    rope_scaling: Dict
    sliding_window: Optional[int]
    tie_word_embeddings: bool


def read_config(model_dir: str) -> Dict:
    path = os.path.join(model_dir, "config.json")
    try:
        with open(path) as f:
            return json.load(f)
    except (OSError, ValueError) as e:
        raise CalibrationConfigError(f"calibration needs {path}: {e}") from None


def parse_config(cfg: Dict, seq_len: Optional[int] = None, max_id: Optional[int] = None) -> DecoderConfig:
    """The keys the forward reads; refuses (naming the key) what it does not implement."""
    mtype = cfg.get("model_type")
    if mtype not in SUPPORTED:
        raise CalibrationConfigError(f"model_type: calibration knows the decoder layout of {', '.join(SUPPORTED)}; "
                                     f"config.json says {mtype!r}")
    for key in ("hidden_size", "num_hidden_layers", "num_attention_heads", "vocab_size"):
        if not isinstance(cfg.get(key), int) or cfg[key] <= 0:
            raise CalibrationConfigError(f"{key}: missing from config.json or not a positive integer")
    act = cfg.get("hidden_act", "silu")
    if act != "silu":
        raise CalibrationConfigError(f"hidden_act: only 'silu' (SwiGLU) is implemented, config.json says {act!r}")
    heads = cfg["num_attention_heads"]
    kv = cfg.get("num_key_value_heads") or heads
    if heads % kv:
        raise CalibrationConfigError(f"num_key_value_heads: {kv} does not divide num_attention_heads {heads}")
    head_dim = cfg.get("head_dim") or cfg["hidden_size"] // heads
    rope = dict(cfg.get("rope_parameters") or {})
    scaling = dict(cfg.get("rope_scaling") or {})
    rope_type = rope.get("rope_type") or scaling.get("rope_type") or scaling.get("type") or "default"
    if rope_type not in ROPE_TYPES:
        key = "rope_parameters.rope_type" if rope.get("rope_type") else "rope_scaling"
        raise CalibrationConfigError(f"{key}: rope type {rope_type!r} is not implemented ({', '.join(ROPE_TYPES)} are)")
    theta = rope.get("rope_theta", cfg.get("rope_theta", 10000.0))
    if rope.get("partial_rotary_factor", cfg.get("partial_rotary_factor", 1.0)) not in (None, 1, 1.0):
        raise CalibrationConfigError("partial_rotary_factor: only full rotary embeddings are implemented")
    window = cfg.get("sliding_window")
    if mtype == "qwen2" and not cfg.get("use_sliding_window", False):
        window = None
    max_pos = cfg.get("max_position_embeddings")
    if seq_len is not None:
        if window is not None and window < seq_len:
            raise CalibrationConfigError(f"sliding_window: {window} is smaller than the sequence length {seq_len} "
                                         f"(windowed attention is not implemented)")
        if max_pos is not None and seq_len > max_pos:
            raise CalibrationConfigError(f"max_position_embeddings: the sequence length {seq_len} exceeds {max_pos}")
    if max_id is not None and max_id >= cfg["vocab_size"]:
        raise CalibrationConfigError(f"vocab_size: input ids reach {max_id}, the vocabulary has {cfg['vocab_size']}")
    merged = {**scaling, **rope}
    return DecoderConfig(mtype, cfg["hidden_size"], cfg["num_hidden_layers"], heads, kv, head_dim, cfg["vocab_size"],
                         max_pos, float(cfg.get("rms_norm_eps", 1e-6)), float(theta), rope_type, merged, window,
                         bool(cfg.get("tie_word_embeddings", False)))


def rope_inv_freq(c: DecoderConfig, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Inverse frequencies [head_dim / 2] — transformers' ROPE_INIT_FUNCTIONS 'default' and 'llama3'
    restated (fp32 as transformers computes them; float64 for a float64 forward)."""
    dim = c.head_dim
    inv = 1.0 / (c.rope_theta ** (torch.arange(0, dim, 2, dtype=torch.int64).to(dtype) / dim))
    if c.rope_type == "default":
        return inv
    p = c.rope_scaling
    try:
        factor, low, high = p["factor"], p["low_freq_factor"], p["high_freq_factor"]
        old_len = p["original_max_position_embeddings"]
    except KeyError as e:
        raise CalibrationConfigError(f"rope_scaling: llama3 needs {e.args[0]}") from None
    low_wavelen, high_wavelen = old_len / low, old_len / high
    wavelen = 2 * math.pi / inv
    scaled = torch.where(wavelen > low_wavelen, inv / factor, inv)
    smooth = (old_len / wavelen - low) / (high - low)
    smoothed = (1 - smooth) * scaled / factor + smooth * scaled
    medium = ~(wavelen < high_wavelen) & ~(wavelen > low_wavelen)
    return torch.where(medium, smoothed, scaled)


def rope_tables(c: DecoderConfig, seq_len: int, dtype: torch.dtype, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos, sin [seq, head_dim] in the compute dtype (angles in fp32 as transformers; fp64 for fp64)."""
    ft = torch.float64 if dtype == torch.float64 else torch.float32
    inv = rope_inv_freq(c, ft).to(device)
    ang = torch.arange(seq_len, device=device).to(ft)[:, None] * inv[None, :]
    emb = torch.cat((ang, ang), dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def rotate_half(x: torch.Tensor) -> torch.Tensor:
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


# ---------------------------------------------------------------- the injected ops
class HipOps:
    """The product's ops: fused HIP kernels, accumulators on the device (no CPU fallback)."""

    def __init__(self, device):
        from .. import _hip
        from .stats import StatsAccumulator
        self._hip, self._acc_cls = _hip, StatsAccumulator
        self.device = torch.device(device)
        _hip.require_device(self.device)

    def new_acc(self, K: int):
        return self._acc_cls(K, self.device)

    def rmsnorm(self, x: torch.Tensor, weight: torch.Tensor, eps: float, acc, fused: bool) -> torch.Tensor:
        if acc is not None and fused and acc.fusable():
            out = self._hip.rmsnorm_stats(x, weight, eps, acc.tokens, acc.acc_abs, acc.acc_sq)
            acc.added(x.shape[0])
            return out
        out = self._hip.rmsnorm_stats(x, weight, eps)
        if acc is not None:
            acc.add(out)
        return out

    def swiglu(self, gate: torch.Tensor, up: torch.Tensor, acc, fused: bool) -> torch.Tensor:
        if acc is None:
            return self._hip.swiglu_stats(gate, up)
        if fused and acc.fusable():
            out = self._hip.swiglu_stats(gate, up, acc.tokens, acc.acc_abs, acc.acc_sq)
            acc.added(gate.shape[0])
            return out
        out = self._hip.swiglu_stats(gate, up)
        acc.add(out)
        return out

    def accum(self, x: torch.Tensor, acc) -> None:
        if acc is not None:
            acc.add(x)


# ---------------------------------------------------------------- the driver
def plan_micro_batches(n: int, seq: int, batch_tokens: int) -> Tuple[List[Tuple[int, int]], bool]:
    """[(first sample, end sample)], and whether every micro-batch but the last has a multiple of
    256 tokens (then the fused kernels may add to the running sums directly)."""
    per = max(1, batch_tokens // seq)
    need = 256 // math.gcd(seq, 256)          # sequences per whole number of 256-token blocks
    if per >= need:
        per = per // need * need
    spans = [(i, min(i + per, n)) for i in range(0, n, per)]
    fused = all((b - a) * seq % 256 == 0 for a, b in spans[:-1])
    return spans, fused


def sample_rows(total: int, n: int) -> List[int]:
    """The token rows kept as samples: t_j = floor(j * total / n) for j < n — evenly spread over the
    token-major activation, ascending, distinct (n is cut to total); n <= 0 keeps nothing."""
    n = min(int(n), int(total))
    return [j * total // n for j in range(n)] if n > 0 else []


def _linear_names(prefix: str, names) -> Dict[str, List[str]]:
    out = {}
    for group, mods in BLOCK_LINEARS:
        out[group] = [f"{prefix}.{m}.weight" for m in mods if f"{prefix}.{m}.weight" in names]
    return out


def run_decoder(loader, cfg: DecoderConfig, input_ids: torch.Tensor, dtype: torch.dtype, device, ops,
                batch_tokens: int = 8192, readers: int = 4, logger=None, n_sample_tokens: int = 0,
                samples_out: Optional[Dict[str, torch.Tensor]] = None, stats: bool = True,
                hidden_out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """The block-by-block pass.  Returns weight name -> (x_mean, x_sq) (fp32, on the CPU).
    n_sample_tokens > 0 also keeps, per block and distinct input, the rows sample_rows(n * seq,
    n_sample_tokens) of the token-major activation (the tensors the producers return, compute
    dtype, gathered per micro-batch) in samples_out["<block prefix>.<group>.samples"] (CPU);
    0 keeps nothing and changes nothing.
    stats=False takes no statistics (every accumulator handed to `ops` is None, the result is empty
    and the final norm is left to the caller); hidden_out, when given, receives the resident hidden
    states after the last block, before the final norm, as hidden_out["hidden"] ([n * seq, H],
    compute dtype, on the device).  Both are for the evaluation pass (awq_quantizer.evaluation)."""
    device = torch.device(device)
    index = {i.name: i for i in loader.tensor_index()}
    root = "model." if "model.embed_tokens.weight" in index else ""
    need = [f"{root}embed_tokens.weight"] + [f"{root}layers.{i}.input_layernorm.weight" for i in range(cfg.num_layers)]
    missing = [n for n in need if n not in index]
    if missing:
        raise CalibrationConfigError(f"checkpoint lacks {missing[0]} (a {cfg.model_type} decoder with "
                                     f"{cfg.num_layers} layers was expected)")
    n, seq = input_ids.shape
    spans, fused = plan_micro_batches(n, seq, batch_tokens)
    H, nh, nkv, hd = cfg.hidden_size, cfg.num_heads, cfg.num_kv_heads, cfg.head_dim

    def fetch(names):
        return {k: loader.read(index[k]) for k in names}

    def block_names(i):
        p = f"{root}layers.{i}."
        return [k for k in index if k.startswith(p)]

    def dev(t):
        return t.to(device=device, dtype=dtype, non_blocking=True)

    results: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
    keep = torch.tensor(sample_rows(n * seq, n_sample_tokens if samples_out is not None else 0), dtype=torch.int64,
                        device=device)

    def publish(acc, names):
        if names:
            m, s = acc.finish()
            m, s = m.float().cpu(), s.float().cpu()
            for k in names:
                results[k] = (m, s)

    with torch.no_grad(), ThreadPoolExecutor(max_workers=max(1, readers)) as pool:
        nxt = pool.submit(fetch, block_names(0))
        embed = dev(loader.read(index[f"{root}embed_tokens.weight"]))
        hidden = F.embedding(input_ids.to(device), embed).reshape(n * seq, H)     # resident, compute dtype
        del embed
        cos, sin = rope_tables(cfg, seq, dtype, device)
        for i in range(cfg.num_layers):
            host = nxt.result()
            if i + 1 < cfg.num_layers:
                nxt = pool.submit(fetch, block_names(i + 1))
            p = f"{root}layers.{i}"
            w = {k[len(p) + 1:]: dev(t) for k, t in host.items()}
            lin = _linear_names(p, index)
            wq, wk, wv = (w[f"self_attn.{m}_proj.weight"] for m in "qkv")
            w_qkv = torch.cat([wq, wk, wv])
            b_qkv = None
            if "self_attn.q_proj.bias" in w:
                b_qkv = torch.cat([w[f"self_attn.{m}_proj.bias"] for m in "qkv"])
            w_gu = torch.cat([w["mlp.gate_proj.weight"], w["mlp.up_proj.weight"]])
            b_gu = None
            if "mlp.gate_proj.bias" in w:
                b_gu = torch.cat([w["mlp.gate_proj.bias"], w["mlp.up_proj.bias"]])
            inter = w["mlp.gate_proj.weight"].shape[0]
            accs = {"attn_in": ops.new_acc(H), "attn_out": ops.new_acc(w["self_attn.o_proj.weight"].shape[1]),
                    "mlp_in": ops.new_acc(H), "mlp_out": ops.new_acc(inter)} if stats else dict.fromkeys(
                        ("attn_in", "attn_out", "mlp_in", "mlp_out"))
            kept = {g: [] for g in accs}
            for a, b in spans:
                x = hidden[a * seq:b * seq]                       # [T, H] view of the resident states
                m = b - a
                sel = keep[(keep >= a * seq) & (keep < b * seq)] - a * seq if keep.numel() else None

                def take(group, t):
                    if sel is not None and sel.numel():
                        kept[group].append(t.index_select(0, sel))

                hn = ops.rmsnorm(x, w["input_layernorm.weight"], cfg.eps, accs["attn_in"], fused)
                take("attn_in", hn)
                qkv = F.linear(hn, w_qkv, b_qkv).view(m, seq, nh + 2 * nkv, hd).transpose(1, 2)
                q, k, v = qkv[:, :nh], qkv[:, nh:nh + nkv], qkv[:, nh + nkv:]
                q = q * cos + rotate_half(q) * sin
                k = k * cos + rotate_half(k) * sin
                if nkv != nh:                                     # kv head j serves query heads j*rep .. j*rep+rep-1
                    k = k.repeat_interleave(nh // nkv, dim=1)
                    v = v.repeat_interleave(nh // nkv, dim=1)
                att = F.scaled_dot_product_attention(q, k, v, is_causal=True)
                att = att.transpose(1, 2).reshape(m * seq, nh * hd)
                ops.accum(att, accs["attn_out"])
                take("attn_out", att)
                x += F.linear(att, w["self_attn.o_proj.weight"], w.get("self_attn.o_proj.bias"))
                hn = ops.rmsnorm(x, w["post_attention_layernorm.weight"], cfg.eps, accs["mlp_in"], fused)
                take("mlp_in", hn)
                gu = F.linear(hn, w_gu, b_gu)                     # [T, 2 * inter]: gate | up
                act = ops.swiglu(gu[:, :inter], gu[:, inter:], accs["mlp_out"], fused)
                take("mlp_out", act)
                x += F.linear(act, w["mlp.down_proj.weight"], w.get("mlp.down_proj.bias"))
            for group, acc in accs.items():
                if acc is not None:
                    publish(acc, lin[group])
                if kept[group]:
                    samples_out[f"{p}.{group}.samples"] = torch.cat(kept[group]).cpu()
            if logger:
                logger.info(f"Calibrated block: {p}" if stats else f"Ran block: {p}")
        if hidden_out is not None:
            hidden_out["hidden"] = hidden
        if stats and "lm_head.weight" in index:
            wn = dev(loader.read(index[f"{root}norm.weight"]))
            acc = ops.new_acc(H)
            for a, b in spans:
                ops.rmsnorm(hidden[a * seq:b * seq], wn, cfg.eps, acc, fused)
            publish(acc, ["lm_head.weight"])
    return results
