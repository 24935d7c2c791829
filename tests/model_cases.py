"""Shared by tests/test_model_forward_host.py and tests/test_gpu_model_forward.py: the fixtures of
tests/golden/model_<arch>/, a textbook float64 RTN (the reference the written checkpoints are
measured against — never the code under test), a packer of the published GEMM layout, a host-side
fold, and the mutations that the tests must be able to catch.  No awq_quantizer, no oracle."""
import functools
import json
import os
import re
from typing import Dict

import torch

from checkpoint_reader import IDENTITY, ORDER, dequant_gemm
from model_forward import model_forward, rel_error

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARCHS = ("llama", "mistral", "qwen2")
BLOCK_LINEAR = re.compile(r"^model\.layers\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj)\.weight$")

# Bounds (derivations: DESIGN.md "Written checkpoints against a full-model forward").
# THETA: a written RTN / activation-aware checkpoint's logit error e stays below THETA * e_textbook.
# The geometric mean of 1 and the smallest layout / zero-point mutation ratio measured on the CPU
# at group sizes 32 and 64 (zero point + 1 on qwen2 at 32: 7.19, sqrt = 2.68), rounded down;
# test_model_forward_host.py re-measures the ratios and fails if one no longer exceeds it.
THETA = 2.6


def fold_bound(fx: "Fixture", dtype: torch.dtype) -> float:
    """Bound on e of a fold's unquantized counterpart: only the rounding of the folded tensors that
    are WRITTEN in the directory's dtype remains — the norm weights (two per layer) and the v_proj
    biases (one per layer with a bias and a foldable attn_out); the linears are formed in float64.
    Each is off by <= 2^-9 (bf16) per element, added coherently over the n tensors on the path:
    n * 2^-9 (llama / mistral 4 -> 2^-7, qwen2 6 -> 1.17e-2), never above the 2^-6 that eight
    rounded folds would give.  fp32: 3e-6 (n * 2^-24 = 3.6e-7 elementwise, 8x for amplification)."""
    n = 2 * fx.layers + (fx.layers if fx.mha and "model.layers.0.self_attn.v_proj.bias" in fx.names else 0)
    return {torch.float32: 3e-6, torch.bfloat16: min(n * 2.0 ** -9, 2.0 ** -6)}[dtype]



class Fixture:
    def __init__(self, arch: str):
        from safetensors.torch import load_file
        self.arch = arch
        self.dir = os.path.join(GOLDEN, f"model_{arch}")
        self.state = load_file(os.path.join(self.dir, "model.safetensors"))          # bf16
        self.stats_path = os.path.join(self.dir, "stats.safetensors")
        self.stats = load_file(self.stats_path)
        ex = load_file(os.path.join(self.dir, "expect.safetensors"))
        self.input_ids, self.logits = ex["input_ids"], ex["logits"]
        with open(os.path.join(self.dir, "config.json")) as f:
            self.config = json.load(f)
        with open(os.path.join(self.dir, "names.json")) as f:
            self.names = {k: tuple(v) for k, v in json.load(f).items()}
        self.source = {k: v.double() for k, v in self.state.items()}
        self.layers = int(self.config["num_hidden_layers"])
        self.mha = self.config["num_key_value_heads"] == self.config["num_attention_heads"]

    def e(self, state: Dict[str, torch.Tensor]) -> float:
        """||logits(state) - logits_ref||_F / ||logits_ref||_F on the fixture's input_ids."""
        return rel_error(model_forward(state, self.config, self.input_ids), self.logits)

    def quantized_names(self, fmt: str):
        """autoawq: the decoder blocks' nn.Linear weights; packed: every tensor (all have >= 128 elements)."""
        return [n for n in self.names if fmt == "packed" or BLOCK_LINEAR.match(n)]


@functools.lru_cache(maxsize=None)
def fixture(arch: str) -> Fixture:
    return Fixture(arch)


# ------------------------------------------------------------------ textbook RTN
def textbook_rtn(w: torch.Tensor, group_size: int):
    """Asymmetric 4-bit min/max RTN in float64 over groups of group_size along the last axis:
    scale = (max - min) / 15, z = round(-min / scale), q = clamp(round(w / scale) + z, 0, 15).
    Returns (q, z, scale) as float64 [rows, K], [rows, G], [rows, G]."""
    w2 = w.double().reshape(-1 if w.dim() > 1 else 1, w.shape[-1])
    rows, K = w2.shape
    g = w2.reshape(rows, K // group_size, group_size)
    mn, mx = g.amin(-1), g.amax(-1)
    scale = (mx - mn) / 15.0
    scale = torch.where(scale == 0, torch.ones_like(scale), scale)
    z = torch.clamp(torch.round(-mn / scale), 0, 15)
    q = torch.clamp(torch.round(g / scale[..., None]) + z[..., None], 0, 15)
    return q.reshape(rows, K), z, scale


def textbook_dequant(w: torch.Tensor, group_size: int) -> torch.Tensor:
    q, z, s = textbook_rtn(w, group_size)
    rows, K = q.shape
    g = q.reshape(rows, K // group_size, group_size)
    return ((g - z[..., None]) * s[..., None]).reshape(w.shape)


@functools.lru_cache(maxsize=None)
def e_textbook(arch: str, fmt: str = "autoawq", group_size: int = 32) -> float:
    fx = fixture(arch)
    state = dict(fx.source)
    for n in fx.quantized_names(fmt):
        state[n] = textbook_dequant(fx.source[n], group_size)
    return fx.e(state)


# ------------------------------------------------------------------ the published GEMM layout, packed
def pack_gemm(q: torch.Tensor, z: torch.Tensor):
    """q [N, K], z [N, G] (values 0 .. 15) -> qweight int32 [K, N/8], qzeros int32 [G, N/8]:
    nibble i of word c = column 8c + ORDER[i]."""
    def pack(cols):                                         # [R, N]
        c = cols.to(torch.int64).reshape(cols.shape[0], -1, 8)[..., list(ORDER)]
        word = (c << torch.arange(0, 32, 4, dtype=torch.int64)).sum(-1)
        return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)
    return pack(q.t()), pack(z.t())


def textbook_gemm(fx: Fixture, group_size: int) -> Dict[str, dict]:
    """name -> {qweight, qzeros, scales (float64)} of the textbook RTN of every block linear."""
    out = {}
    for n in fx.quantized_names("autoawq"):
        q, z, s = textbook_rtn(fx.source[n], group_size)
        qw, qz = pack_gemm(q, z)
        out[n] = {"qweight": qw, "qzeros": qz, "scales": s.t().contiguous()}
    return out


def layout_mutations(fx: Fixture, gemm: Dict[str, dict], group_size: int, rest: Dict[str, torch.Tensor]):
    """The states a reader with the wrong nibble order / a zero point off by one would see.
    gemm: name -> GEMM-layout tensors; rest: every other tensor (float64).  Also "none"."""
    out = {}
    for label, kw in (("none", {}), ("identity_nibble_order", {"order": IDENTITY}),
                      ("zero_point_plus_1", {"zero_shift": 1})):
        state = dict(rest)
        for n, r in gemm.items():
            state[n] = dequant_gemm(r["qweight"], r["qzeros"], r["scales"], group_size, **kw)
        out[label] = state
    return out


# ------------------------------------------------------------------ folds
def unquantized_fold(fx: Fixture, scales: Dict[str, torch.Tensor], written: Dict[str, torch.Tensor],
                     invert_mlp_out: bool = False) -> Dict[str, torch.Tensor]:
    """The unquantized counterpart of a --fold_scales checkpoint: every member linear
    W_src * diag(input_scale) / row_scale in float64 (scales: awq_scales.safetensors' tensors), every
    other tensor as `written` holds it (folded norm weights and biases included).
    invert_mlp_out: every up_proj's rows multiplied by s where they belong divided."""
    state = {k: v.double() for k, v in written.items()}
    for n in fx.quantized_names("autoawq"):
        w = fx.source[n]
        if n + ".input_scale" in scales:
            w = w * scales[n + ".input_scale"].double()[None, :]
        if n + ".row_scale" in scales:
            rs = scales[n + ".row_scale"].double()[:, None]
            w = w * rs if invert_mlp_out and n.endswith(".mlp.up_proj.weight") else w / rs
        state[n] = w
    return state


def host_fold(fx: Fixture, dtype: torch.dtype):
    """A fold made on the host from the fixture's statistics, s = sqrt(x_mean) normalised by
    sqrt(max * min) (the published search's ratio 1/2 without the weight term): (scales in the
    sidecar's naming, written = the source with the folded norm weights / biases rounded to dtype)."""
    scales, written = {}, {k: v.to(dtype) for k, v in fx.state.items()}

    def s_of(member):
        xm = fx.stats[member + ".x_mean"].double().clamp_min(1e-4).sqrt()
        return (xm / (xm.max() * xm.min()).sqrt()).float()

    def fold(name, s):
        written[name] = (fx.source[name] / s.double().reshape([-1] + [1] * (fx.source[name].dim() - 1))).to(dtype)

    for i in range(fx.layers):
        p = f"model.layers.{i}"
        groups = [(("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "input_layernorm", False),
                  (("mlp.gate_proj", "mlp.up_proj"), "post_attention_layernorm", False),
                  (("mlp.down_proj",), "mlp.up_proj", True)]
        if fx.mha:
            groups.append((("self_attn.o_proj",), "self_attn.v_proj", True))
        for members, producer, rows in groups:
            s = s_of(f"{p}.{members[0]}.weight")
            for m in members:
                scales[f"{p}.{m}.weight.input_scale"] = s
            if rows:
                scales[f"{p}.{producer}.weight.row_scale"] = s
                if f"{p}.{producer}.bias" in fx.source:
                    fold(f"{p}.{producer}.bias", s)
            else:
                fold(f"{p}.{producer}.weight", s)
    return scales, written


def fold_mutations(fx: Fixture, scales, written) -> Dict[str, Dict[str, torch.Tensor]]:
    """"none" and the wrong folds: one source norm weight kept where the folded one belongs, the
    mlp_out fold inverted, and (a model with a v_proj bias and a folded attn_out) the bias fold dropped."""
    out = {"none": unquantized_fold(fx, scales, written)}
    norm = "model.layers.0.input_layernorm.weight"
    out["source_norm_kept"] = unquantized_fold(fx, scales, {**written, norm: fx.state[norm]})
    out["mlp_out_fold_inverted"] = unquantized_fold(fx, scales, written, invert_mlp_out=True)
    biases = [n for n in fx.source if n.endswith("self_attn.v_proj.bias")
              and n[: -len("bias")] + "weight.row_scale" in scales]
    if biases:
        out["v_bias_fold_dropped"] = unquantized_fold(fx, scales, {**written, **{b: fx.state[b] for b in biases}})
    return out
