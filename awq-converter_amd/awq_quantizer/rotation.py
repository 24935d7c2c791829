"""Hadamard rotation of a Llama-layout checkpoint: the residual stream is rotated
by Q = diag(d) H_h / sqrt(h) and the rotation folded into the weights, so the rotated directory is a
plain checkpoint of the same function whose outliers are spread over all channels (QuaRot's R1 / R2).

Row-vector convention, weights [out, in].  h = m 2^k, H_h = M_m (x) H_{2^k} (Sylvester), M_1 = [1],
M_12 / M_20 Paley I (q = 11 / 19), M_28 Paley II (q = 13); d in {+-1}^h from a seeded generator.
The transforms are the HIP kernels awq_hadamard_rows / awq_hadamard_cols; there is no torch path.
"""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from .quantization.block_plan import SUPPORTED

MAX_LENGTH = 16384          # include/awq_hip.h: L <= 16384, 2^k >= 16
_PALEY = {3: (12, 11), 5: (20, 19), 7: (28, 13)}       # odd part of n -> (m, q)


def _jacobsthal(q: int) -> torch.Tensor:
    """Q[i][j] = chi(i - j), chi the quadratic character of GF(q), q prime."""
    squares = {(x * x) % q for x in range(1, q)}
    chi = [0] + [1 if a in squares else -1 for a in range(1, q)]
    return torch.tensor([[chi[(i - j) % q] for j in range(q)] for i in range(q)], dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _mix_matrix(m: int) -> Optional[torch.Tensor]:
    if m == 1:
        return None
    q = {12: 11, 20: 19, 28: 13}[m]
    Q, one = _jacobsthal(q), torch.ones(q, dtype=torch.float64)
    S = torch.zeros(q + 1, q + 1, dtype=torch.float64)
    S[0, 1:], S[1:, 1:] = one, Q
    if q % 4 == 3:                                     # Paley I: I + S, S skew
        S[1:, 0] = -one
        M = torch.eye(q + 1, dtype=torch.float64) + S
    else:                                              # Paley II: S symmetric, order 2 (q + 1)
        S[1:, 0] = one
        a = torch.tensor([[1.0, 1.0], [1.0, -1.0]], dtype=torch.float64)
        b = torch.tensor([[1.0, -1.0], [-1.0, -1.0]], dtype=torch.float64)
        M = torch.kron(S, a) + torch.kron(torch.eye(q + 1, dtype=torch.float64), b)
    assert M.shape == (m, m) and bool((M.abs() == 1).all()) and torch.equal(M @ M.T, m * torch.eye(m, dtype=torch.float64))
    return M


def hadamard_factor(n: int) -> Tuple[int, int, Optional[torch.Tensor]]:
    """n = m 2^k with m in {1, 12, 20, 28} and 2^k >= 16: (m, k, M), M the float64 m x m Hadamard matrix
    (None for m = 1).  Raises ValueError for any other n."""
    n = int(n)
    odd, e = n, 0
    while odd > 1 and odd % 2 == 0:
        odd, e = odd // 2, e + 1
    m = 1 if odd == 1 else _PALEY.get(odd, (0, 0))[0]
    k = e if m == 1 else e - 2
    if n < 1 or m == 0 or k < 4 or n > MAX_LENGTH:
        raise ValueError(f"no Hadamard transform of length {n}: it must be m * 2^k with m in (1, 12, 20, 28), "
                         f"2^k >= 16 and at most {MAX_LENGTH}")
    return m, k, _mix_matrix(m)


_mix_on_device: Dict[Tuple[int, str], torch.Tensor] = {}


def _device_mix(m: int, device: torch.device) -> Optional[torch.Tensor]:
    if m == 1:
        return None
    key = (m, str(device))
    if key not in _mix_on_device:
        _mix_on_device[key] = _mix_matrix(m).to(torch.float32).to(device).contiguous()
    return _mix_on_device[key]


def hadamard_transform(x: torch.Tensor, dim: int, *, length: Optional[int] = None,
                       pre: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The orthonormal Hadamard transform of a 2-D bf16 / fp16 / fp32 device tensor along `dim`, in
    consecutive segments of `length` (default: the whole axis), H = M (x) H_{2^k} of hadamard_factor:
      dim = -1:  out_seg = ((x_seg * pre_seg) H) / sqrt(length)        (awq_hadamard_rows)
      dim = 0:   out_seg = H^T (pre_seg * x_seg) / sqrt(length)        (awq_hadamard_cols; columns % 8 == 0)
    pre: optional fp32 vector, one factor per index along `dim`.  Returns a new tensor."""
    from . import _hip
    if x.dim() != 2 or dim not in (0, 1, -1):
        raise ValueError("hadamard_transform takes a 2-D tensor and dim 0 or -1")
    if x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise ValueError(f"hadamard_transform takes bf16 / fp16 / fp32 tensors, got {x.dtype}")
    axis = 0 if dim == 0 else 1
    n = x.shape[axis]
    L = n if length is None else int(length)
    m, _, _ = hadamard_factor(L)
    if n % L:
        raise ValueError(f"length {L} does not divide the axis ({n})")
    _hip.require_device(x.device)
    x = x.contiguous()
    if pre is not None:
        if pre.numel() != n:
            raise ValueError(f"pre must hold {n} factors")
        pre = pre.to(device=x.device, dtype=torch.float32).contiguous()
    out = torch.empty_like(x)
    (_hip.hadamard_cols if axis == 0 else _hip.hadamard_rows)(x, L, m, pre, _device_mix(m, x.device), out)
    return out


# ------------------------------------------------------------------ the plan
@dataclass
class Op:
    kind: str                       # "rows" (W diag(g) Q), "cols" (Q^T W), "copy", "ones" (a folded norm weight)
    norm: Optional[str] = None      # rows: the norm weight g that is folded in (None: pre = d alone)
    head: Optional[str] = None      # --rotate_heads: "cols" / "rows", a second pass in head_dim segments
    source: Optional[str] = None    # the tensor that is read, when it is not the one written (tied lm_head)


@dataclass
class RotationPlan:
    h: int
    m: int
    k: int
    head_dim: int
    ops: Dict[str, Op]
    ones: List[str]
    tied: bool                      # lm_head.weight is created from embed_tokens; tie_word_embeddings becomes false

    def by_operation(self, heads: bool) -> Dict[str, List[str]]:
        out: Dict[str, List[str]] = {}
        for name, op in self.ops.items():
            key = op.kind + (f"+head_{op.head}" if heads and op.head else "")
            out.setdefault(key, []).append(name)
        return out


_LAYER = re.compile(r"^(model\.layers\.\d+)\.(.+)$")
_READS = {"self_attn.q_proj": "input_layernorm", "self_attn.k_proj": "input_layernorm",
          "self_attn.v_proj": "input_layernorm", "mlp.gate_proj": "post_attention_layernorm",
          "mlp.up_proj": "post_attention_layernorm"}
_WRITES = ("self_attn.o_proj", "mlp.down_proj")


def plan_rotation(shapes: Dict[str, Tuple[int, ...]], config: dict) -> RotationPlan:
    """shapes: tensor name -> shape of the whole checkpoint; config: config.json.  Pure Python."""
    mt = config.get("model_type")
    if mt not in SUPPORTED:
        raise ValueError(f"rotation knows the layout of model types {', '.join(SUPPORTED)}; got {mt!r}")
    h = int(config["hidden_size"])
    m, k, _ = hadamard_factor(h)
    heads = int(config["num_attention_heads"])
    hd = int(config.get("head_dim") or h // heads)
    hadamard_factor(hd)
    embed, final, lm = "model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"
    for need in (embed, final):
        if need not in shapes:
            raise ValueError(f"rotation needs {need}")
    ops: Dict[str, Op] = {}
    ones: List[str] = []

    def need_norm(name: str) -> str:
        if tuple(shapes.get(name, ())) != (h,):
            raise ValueError(f"rotation needs the norm weight {name} of shape ({h},)")
        if name not in ones:
            ones.append(name)
        return name

    for name, shape in shapes.items():
        shape = tuple(shape)
        lay = _LAYER.match(name)
        if name == embed:
            ops[name] = Op("rows")
        elif name == lm:
            ops[name] = Op("rows", norm=need_norm(final))
        elif lay and lay.group(2).endswith(".weight") and lay.group(2)[:-7] in _READS:
            mod = lay.group(2)[:-7]
            if len(shape) != 2 or shape[1] != h:
                raise ValueError(f"{name} {shape} does not read a residual stream of {h} channels")
            v = mod == "self_attn.v_proj"
            if v and shape[0] % hd:
                raise ValueError(f"{name} {shape}: rows are no multiple of head_dim {hd}")
            ops[name] = Op("rows", norm=need_norm(f"{lay.group(1)}.{_READS[mod]}.weight"), head="cols" if v else None)
        elif lay and lay.group(2).endswith(".weight") and lay.group(2)[:-7] in _WRITES:
            o = lay.group(2)[:-7] == "self_attn.o_proj"
            if len(shape) != 2 or shape[0] != h or shape[1] % 8 or (o and shape[1] % hd):
                raise ValueError(f"{name} {shape} does not write a residual stream of {h} channels")
            ops[name] = Op("cols", head="rows" if o else None)
        elif lay and lay.group(2)[:-5] in _WRITES and lay.group(2).endswith(".bias"):
            ops[name] = Op("rows")                      # b Q
        elif lay and lay.group(2) == "self_attn.v_proj.bias":
            ops[name] = Op("copy", head="rows")         # b H_d per head, --rotate_heads only
        else:
            ops[name] = Op("copy")
    tied = lm not in shapes
    if tied:
        ops[lm] = Op("rows", norm=need_norm(final), source=embed)
    for n in ones:
        ops[n] = Op("ones")
    return RotationPlan(h, m, k, hd, ops, ones, tied)


def rotation_signs(h: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randint(0, 2, (h,), generator=g) * 2 - 1).to(torch.float32)


def apply_op(op: Op, w: torch.Tensor, plan: RotationPlan, d: torch.Tensor, g: Optional[torch.Tensor], heads: bool,
             device: torch.device) -> torch.Tensor:
    """One tensor of the plan: w in the dtype it is written in, d the signs (fp32, on the device), g the
    norm weight of op.norm.  A tensor that takes two passes is kept fp32 between them and rounded once."""
    if op.kind == "ones":
        return torch.ones_like(w)
    head = op.head if heads else None
    if op.kind == "copy" and not head:
        return w
    x = w.to(device)
    vec = x.dim() == 1
    if vec:
        x = x.reshape(1, -1)
    two = op.kind != "copy" and head is not None
    y = x.float() if two else x
    if op.kind == "rows":
        y = hadamard_transform(y, -1, pre=d if g is None else g.to(device=device, dtype=torch.float32) * d)
    elif op.kind == "cols":
        y = hadamard_transform(y, 0, pre=d)
    if head:
        y = hadamard_transform(y, 0 if head == "cols" else -1, length=plan.head_dim)
    y = y.to(w.dtype)
    return (y.reshape(-1) if vec else y).cpu()


def rotate_state(state: Dict[str, torch.Tensor], config: dict, seed: int = 0, heads: bool = False,
                 device="cuda") -> Dict[str, torch.Tensor]:
    """The rotated state dict (CPU tensors, each in its own dtype): plan_rotation applied with the
    signs of `seed`; with a tied embedding lm_head.weight is added."""
    device = torch.device(device)
    plan = plan_rotation({n: tuple(t.shape) for n, t in state.items()}, config)
    d = rotation_signs(plan.h, seed).to(device)
    out = {}
    for name, op in plan.ops.items():
        g = state[op.norm] if op.norm else None
        out[name] = apply_op(op, state[op.source or name], plan, d, g, heads, device)
    return out
