"""Which tensors of a checkpoint are nn.Linear weights an AutoAWQ checkpoint quantizes — a
heuristic on names and shapes (a checkpoint has no module graph), shared by the CLI's AutoAWQ
export (main.py) and the block plan (block_plan.py)."""
from typing import Optional, Tuple

_NOT_LINEAR = ("embed", "lm_head", "norm", "wte", "wpe", "ln_", "router")
# model types whose projection weights are transformers Conv1D modules, stored [in, out]
# (quantizing them as [out, in] would group along the wrong axis): copied, not quantized
CONV1D_MODEL_TYPES = ("gpt2", "openai-gpt", "imagegpt", "decision_transformer")


def is_linear_shape(name: str, shape: Tuple[int, ...], group_size: int, model_type: Optional[str] = None) -> bool:
    """is_linear_weight without the dtype (a name / shape table carries none)."""
    if len(shape) != 2 or not name.endswith(".weight"):
        return False
    if model_type in CONV1D_MODEL_TYPES:
        return False
    if any(s in name for s in _NOT_LINEAR) or name.endswith(".gate.weight"):
        return False
    n, k = shape
    return n % 8 == 0 and k % group_size == 0


def is_linear_weight(info, group_size: int, model_type: Optional[str] = None) -> bool:
    """The tensors an AutoAWQ checkpoint quantizes: 2-D `*.weight` of nn.Linear layers whose
    shape the GEMM layout can hold.  Heuristic on names (no module graph in a checkpoint):
    not embeddings, the LM head, norms, MoE routers (`*.router.*`, and `*.gate.weight` —
    Mixtral's block_sparse_moe.gate / Qwen-MoE's mlp.gate; `gate_proj` is a linear) which
    AutoAWQ keeps in fp16, nor any weight of a Conv1D model (CONV1D_MODEL_TYPES).
    info: a TensorInfo (name, shape, dtype)."""
    if len(info.shape) != 2 or not info.dtype.is_floating_point:
        return False
    return is_linear_shape(info.name, info.shape, group_size, model_type)
