"""Layer groups of a decoder block and the ops their searched input scales fold into.

The activation-aware search (act_search.py) quantizes W * diag(s); that is only usable once
1 / s is folded into whatever produces the linear's input, and linears that read ONE input
must share one s.  A checkpoint has no module graph, so the plan is read off Llama tensor
names (model types SUPPORTED); per block prefix `...layers.<i>` (GROUPS, in this order):

  group     members (.weight)                      producer 1 / s folds into
  attn_in   self_attn.q_proj, k_proj, v_proj       input_layernorm.weight (a vector)
  attn_out  self_attn.o_proj                       rows of self_attn.v_proj.weight (+ v_proj.bias);
                                                   only if v_proj.shape[0] == o_proj.shape[1] (with
                                                   GQA shapes the group is not foldable, as in AutoAWQ)
  mlp_in    mlp.gate_proj, up_proj                 post_attention_layernorm.weight
  mlp_out   mlp.down_proj                          rows of mlp.up_proj.weight (+ up_proj.bias)

A group with a member or its producer missing from the checkpoint is not foldable; members must
pass is_linear_weight's name and shape test (linear_weights.py).  OPT, Gemma (its norm is
1 + w), MoE and Conv1D models are out of scope.  Pure Python: no device, no tensor data.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

from .linear_weights import is_linear_shape

SUPPORTED = ("llama", "mistral", "qwen2")

# group -> (member linears, producer, how the producer takes 1 / s)
GROUPS = (
    ("attn_in", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "input_layernorm", "vector"),
    ("attn_out", ("self_attn.o_proj",), "self_attn.v_proj", "rows"),
    ("mlp_in", ("mlp.gate_proj", "mlp.up_proj"), "post_attention_layernorm", "vector"),
    ("mlp_out", ("mlp.down_proj",), "mlp.up_proj", "rows"),
)

_BLOCK_RE = re.compile(r"^(.*\blayers\.\d+)\.")


@dataclass
class Group:
    name: str                       # attn_in / attn_out / mlp_in / mlp_out
    members: List[str]              # the linears (weight names) present in the checkpoint, table order
    producers: List[str]            # tensors 1 / s folds into: [norm weight], or [linear weight(, its bias)]
    fold: str                       # "vector": producers[0] / s;  "rows": producer rows (and bias) / s
    foldable: bool
    reason: str = ""                # why not, when not foldable


@dataclass
class Block:
    prefix: str                     # "...layers.<i>"
    groups: Dict[str, Group] = field(default_factory=dict)

    def members(self) -> List[str]:
        return [m for g in self.groups.values() for m in g.members]

    def tensor_names(self) -> List[str]:
        """Every tensor quantize_block reads: the members, and the producers of foldable groups."""
        names = self.members()
        for g in self.groups.values():
            if g.foldable:
                names += [p for p in g.producers if p not in names]
        return names


class Plan(list):
    """plan_blocks' result: the Blocks (checkpoint order), and `ungrouped`, every linear weight
    that belongs to no group (those keep plain RTN)."""
    ungrouped: List[str]


def plan_blocks(shapes: Dict[str, Tuple[int, ...]], model_type: Optional[str], group_size: int = 128) -> Plan:
    """shapes: tensor name -> shape of the whole checkpoint.  Returns the Plan of its decoder blocks."""
    if model_type not in SUPPORTED:
        raise ValueError(f"scale folding knows the block layout of model types {', '.join(SUPPORTED)}; "
                         f"got {model_type!r}")
    def linear(name: str) -> bool:
        return name in shapes and is_linear_shape(name, tuple(shapes[name]), group_size, model_type)

    prefixes: List[str] = []
    for name in shapes:
        m = _BLOCK_RE.match(name)
        if m and m.group(1) not in prefixes:
            prefixes.append(m.group(1))
    plan = Plan()
    grouped = set()
    for prefix in prefixes:
        block = Block(prefix)
        for gname, member_mods, producer_mod, fold in GROUPS:
            wanted = [f"{prefix}.{m}.weight" for m in member_mods]
            members = [n for n in wanted if linear(n)]
            pw = f"{prefix}.{producer_mod}.weight"
            producers = [pw] if pw in shapes else []
            reason = ""
            if len(members) != len(wanted):
                reason = "missing member: " + ", ".join(n for n in wanted if n not in members)
            elif not producers:
                reason = f"missing producer: {pw}"
            elif fold == "vector":
                if tuple(shapes[pw]) != (shapes[members[0]][1],):
                    reason = f"{pw} {tuple(shapes[pw])} is not a vector of the members' in_features"
            else:
                pb = f"{prefix}.{producer_mod}.bias"
                if pb in shapes:
                    producers.append(pb)
                if not linear(pw):
                    reason = f"producer {pw} is not a quantized linear"
                elif shapes[pw][0] != shapes[members[0]][1]:
                    reason = (f"{pw} has {shapes[pw][0]} rows for {shapes[members[0]][1]} input channels "
                              f"(grouped-query attention): no one-to-one fold")
                elif pb in shapes and tuple(shapes[pb]) != (shapes[pw][0],):
                    reason = f"{pb} {tuple(shapes[pb])} does not match the producer's rows"
            if members:
                block.groups[gname] = Group(gname, members, producers, fold, not reason, reason)
                grouped.update(members)
        if block.groups:
            plan.append(block)
    plan.ungrouped = [n for n in shapes if n not in grouped and linear(n)]
    return plan
