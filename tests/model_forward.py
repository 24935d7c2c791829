"""A plain float64 CPU forward of a Llama-family decoder (llama / mistral / qwen2 tensor names),
from a name -> tensor dict and the config.json dict.  No transformers: it is what the tests run on
a written checkpoint, and tests/test_model_forward_host.py pins it to transformers' own classes
through the logits recorded in tests/golden/model_<arch>/.

RMSNorm with the config's eps, RoPE (rotate-half convention) with the config's theta, grouped-query
attention by repeating kv heads, optional biases on every linear, SwiGLU, the causal mask, the
final norm and lm_head."""
import math
from typing import Dict

import torch


def rope_theta(config: dict) -> float:
    rp = config.get("rope_parameters") or {}
    if "rope_theta" in rp:
        return float(rp["rope_theta"])
    return float(config.get("rope_theta", 10000.0))


def model_forward(state: Dict[str, torch.Tensor], config: dict, input_ids: torch.Tensor) -> torch.Tensor:
    """logits float64 [batch, tokens, vocab]."""
    T = {k: v.double() for k, v in state.items()}
    hid = int(config["hidden_size"])
    heads = int(config["num_attention_heads"])
    kv = int(config.get("num_key_value_heads") or heads)
    hd = int(config.get("head_dim") or hid // heads)
    eps = float(config["rms_norm_eps"])
    B, n = input_ids.shape

    def norm(h, w):
        return h / torch.sqrt((h * h).mean(-1, keepdim=True) + eps) * w

    def lin(h, mod):
        y = h @ T[mod + ".weight"].T
        b = T.get(mod + ".bias")
        return y if b is None else y + b

    inv = rope_theta(config) ** (-torch.arange(0, hd, 2, dtype=torch.float64) / hd)
    ang = torch.arange(n, dtype=torch.float64)[:, None] * inv[None, :]          # [n, hd / 2]
    cos, sin = torch.cat((ang, ang), -1).cos(), torch.cat((ang, ang), -1).sin()

    def rope(x):                                                                  # [B, h, n, hd]
        x1, x2 = x[..., : hd // 2], x[..., hd // 2:]
        return x * cos + torch.cat((-x2, x1), -1) * sin

    mask = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    x = T["model.embed_tokens.weight"][input_ids]
    for i in range(int(config["num_hidden_layers"])):
        p = f"model.layers.{i}"
        h = norm(x, T[f"{p}.input_layernorm.weight"])
        q = rope(lin(h, f"{p}.self_attn.q_proj").reshape(B, n, heads, hd).transpose(1, 2))
        k = rope(lin(h, f"{p}.self_attn.k_proj").reshape(B, n, kv, hd).transpose(1, 2))
        v = lin(h, f"{p}.self_attn.v_proj").reshape(B, n, kv, hd).transpose(1, 2)
        k, v = k.repeat_interleave(heads // kv, dim=1), v.repeat_interleave(heads // kv, dim=1)
        att = (q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(mask, float("-inf")).softmax(-1)
        x = x + lin((att @ v).transpose(1, 2).reshape(B, n, heads * hd), f"{p}.self_attn.o_proj")
        h = norm(x, T[f"{p}.post_attention_layernorm.weight"])
        x = x + lin(torch.nn.functional.silu(lin(h, f"{p}.mlp.gate_proj")) * lin(h, f"{p}.mlp.up_proj"),
                    f"{p}.mlp.down_proj")
    return lin(norm(x, T["model.norm.weight"]), "lm_head")


def rel_error(logits: torch.Tensor, ref: torch.Tensor) -> float:
    """e = ||logits - ref||_F / ||ref||_F."""
    return float((logits.double() - ref.double()).norm() / ref.double().norm())
