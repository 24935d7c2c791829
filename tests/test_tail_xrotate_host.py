"""Hadamard rotation without a GPU: the factorisation h = m 2^k and its Paley
matrices, the plan of the three fixtures (and a tied-embedding variant), and the argument checks of
awq_hadamard_rows / awq_hadamard_cols with nothing launched."""
import ctypes

import pytest
import torch

import model_cases as mc


@pytest.mark.parametrize("n,m,k", [(128, 1, 7), (1536, 12, 7), (5120, 20, 8), (3584, 28, 7), (4096, 1, 12)])
def test_hadamard_factor(n, m, k):
    from awq_quantizer.rotation import hadamard_factor
    got_m, got_k, M = hadamard_factor(n)
    assert (got_m, got_k) == (m, k) and m * 2 ** k == n
    if m > 1:
        assert M.shape == (m, m) and bool((M.abs() == 1).all())
        assert torch.equal(M @ M.T, m * torch.eye(m, dtype=M.dtype))
    else:
        assert M is None
    with pytest.raises(ValueError, match="no Hadamard transform of length 100"):
        hadamard_factor(100)


@pytest.mark.parametrize("arch,tied", [("llama", False), ("mistral", False), ("qwen2", False), ("llama", True)])
def test_plan_assigns_every_tensor_one_operation(arch, tied):
    from awq_quantizer.rotation import plan_rotation
    fx = mc.fixture(arch)
    shapes = {n: s for n, s in fx.names.items() if not (tied and n == "lm_head.weight")}
    plan = plan_rotation(shapes, dict(fx.config, tie_word_embeddings=tied))
    assert (plan.h, plan.m, plan.k, plan.head_dim, plan.tied) == (128, 1, 7, 32, tied)
    assert set(plan.ops) == set(fx.names)                               # lm_head is created when tied
    assert plan.ops["lm_head.weight"].source == ("model.embed_tokens.weight" if tied else None)
    listed = [n for names in plan.by_operation(True).values() for n in names]
    assert sorted(listed) == sorted(fx.names)
    norms = {n for n in fx.names if n.endswith("norm.weight")}
    assert set(plan.ones) == norms == {n for n, op in plan.ops.items() if op.kind == "ones"}
    p = "model.layers.1."
    kinds = {n[len(p):-7]: (op.kind, op.norm and op.norm[len(p):-7], op.head) for n, op in plan.ops.items()
             if n.startswith(p) and n.endswith("proj.weight")}
    assert kinds == {"self_attn.q_proj": ("rows", "input_layernorm", None),
                     "self_attn.k_proj": ("rows", "input_layernorm", None),
                     "self_attn.v_proj": ("rows", "input_layernorm", "cols"),
                     "self_attn.o_proj": ("cols", None, "rows"),
                     "mlp.gate_proj": ("rows", "post_attention_layernorm", None),
                     "mlp.up_proj": ("rows", "post_attention_layernorm", None),
                     "mlp.down_proj": ("cols", None, None)}
    if arch == "qwen2":
        assert plan.ops[p + "self_attn.q_proj.bias"].kind == "copy" and plan.ops[p + "self_attn.v_proj.bias"].head == "rows"
    with pytest.raises(ValueError, match="model types"):
        plan_rotation(shapes, dict(fx.config, model_type="gemma"))
    with pytest.raises(ValueError, match="no Hadamard transform of length 100"):
        plan_rotation(shapes, dict(fx.config, hidden_size=100))


@pytest.mark.parametrize("call,code,word", [
    (lambda l, p: l.awq_hadamard_rows(p, 0, 4, 96, 64, 1, None, None, p, None), 1, "L must divide K"),
    (lambda l, p: l.awq_hadamard_rows(p, 0, 4, 8, 8, 1, None, None, p, None), 1, "2^k >= 16"),
    (lambda l, p: l.awq_hadamard_rows(p, 0, 4, 192, 192, 12, None, None, p, None), 1, "needs the mix matrix"),
    (lambda l, p: l.awq_hadamard_rows(p, 0, 4, 176, 176, 11, None, p, p, None), 2, "1, 12, 20 or 28"),
    (lambda l, p: l.awq_hadamard_rows(p, 3, 4, 64, 64, 1, None, None, p, None), 2, "bf16 / fp16 / fp32"),
    (lambda l, p: l.awq_hadamard_rows(None, 0, 0, 64, 64, 1, None, None, None, None), 0, ""),
    (lambda l, p: l.awq_hadamard_cols(p, 0, 96, 8, 64, 1, None, None, p, None, None), 1, "L must divide K"),
    (lambda l, p: l.awq_hadamard_cols(p, 0, 8, 8, 8, 1, None, None, p, None, None), 1, "2^k >= 16"),
    (lambda l, p: l.awq_hadamard_cols(p, 0, 64, 12, 64, 1, None, None, p, None, None), 1, "N % 8"),
    (lambda l, p: l.awq_hadamard_cols(p, 0, 320, 8, 320, 20, None, None, p, None, None), 1, "needs the mix matrix"),
    (lambda l, p: l.awq_hadamard_cols(p, 0, 4096, 8, 4096, 1, None, None, p, None, None), 1, "needs the workspace"),
    (lambda l, p: l.awq_hadamard_cols(None, 0, 64, 0, 64, 1, None, None, None, None, None), 0, ""),
])
def test_entries_refuse_without_a_launch(call, code, word):
    from awq_quantizer import _hip
    lib = _hip.load_library()
    assert lib.awq_abi_version() == 17
    buf = (ctypes.c_char * 64)()
    assert call(lib, ctypes.cast(buf, ctypes.c_void_p)) == code and word in _hip.last_error()
    assert lib.awq_hadamard_cols_work_bytes(0, 4096, 264, 4096, 1) == 4096 * 264 * 8
    assert lib.awq_hadamard_cols_work_bytes(0, 128, 72, 128, 1) == 0 == lib.awq_hadamard_cols_work_bytes(2, 4096, 264, 4096, 1)
