"""Scale folding without a GPU: the block plan (quantization/block_plan.py), the --fold_scales
flag's refusals (main.py) and awq_fold_rows' argument checks (include/awq_hip.h) — no kernel
is launched here."""
import ctypes
import json
import os

import pytest
import torch
from safetensors.torch import save_file

P = "model.layers"


def llama_shapes(layers=2, hidden=128, inter=256, kv=None, bias=False):
    kv = hidden if kv is None else kv
    sh = {"model.embed_tokens.weight": (512, hidden), "model.norm.weight": (hidden,), "lm_head.weight": (512, hidden)}
    for i in range(layers):
        p = f"{P}.{i}"
        sh.update({f"{p}.input_layernorm.weight": (hidden,), f"{p}.post_attention_layernorm.weight": (hidden,),
                   f"{p}.self_attn.q_proj.weight": (hidden, hidden), f"{p}.self_attn.k_proj.weight": (kv, hidden),
                   f"{p}.self_attn.v_proj.weight": (kv, hidden), f"{p}.self_attn.o_proj.weight": (hidden, hidden),
                   f"{p}.mlp.gate_proj.weight": (inter, hidden), f"{p}.mlp.up_proj.weight": (inter, hidden),
                   f"{p}.mlp.down_proj.weight": (hidden, inter)})
        if bias:
            sh.update({f"{p}.self_attn.q_proj.bias": (hidden,), f"{p}.self_attn.k_proj.bias": (kv,),
                       f"{p}.self_attn.v_proj.bias": (kv,)})
    return sh


def plan(shapes, model_type="llama", group_size=32):
    from awq_quantizer.quantization.block_plan import plan_blocks
    return plan_blocks(shapes, model_type, group_size)


def test_plan_llama_two_layers():
    blocks = plan(llama_shapes())
    assert [b.prefix for b in blocks] == [f"{P}.0", f"{P}.1"]
    for b in blocks:
        p = b.prefix
        assert list(b.groups) == ["attn_in", "attn_out", "mlp_in", "mlp_out"]
        g = b.groups
        assert g["attn_in"].members == [f"{p}.self_attn.{m}_proj.weight" for m in "qkv"]
        assert g["attn_in"].producers == [f"{p}.input_layernorm.weight"] and g["attn_in"].fold == "vector"
        assert g["attn_out"].members == [f"{p}.self_attn.o_proj.weight"]
        assert g["attn_out"].producers == [f"{p}.self_attn.v_proj.weight"] and g["attn_out"].fold == "rows"
        assert g["mlp_in"].members == [f"{p}.mlp.gate_proj.weight", f"{p}.mlp.up_proj.weight"]
        assert g["mlp_in"].producers == [f"{p}.post_attention_layernorm.weight"] and g["mlp_in"].fold == "vector"
        assert g["mlp_out"].members == [f"{p}.mlp.down_proj.weight"]
        assert g["mlp_out"].producers == [f"{p}.mlp.up_proj.weight"] and g["mlp_out"].fold == "rows"
        assert all(x.foldable for x in g.values())
        assert len(b.members()) == 7 and set(b.tensor_names()) == set(b.members()) | {
            f"{p}.input_layernorm.weight", f"{p}.post_attention_layernorm.weight"}
    assert blocks.ungrouped == []


def test_plan_gqa_attn_out_not_foldable():
    (b,) = plan(llama_shapes(layers=1, kv=64))
    assert not b.groups["attn_out"].foldable and "grouped-query" in b.groups["attn_out"].reason
    assert [n for n, g in b.groups.items() if g.foldable] == ["attn_in", "mlp_in", "mlp_out"]


def test_plan_qwen2_biases_are_row_folded_producers():
    (b,) = plan(llama_shapes(layers=1, bias=True), "qwen2")
    p = b.prefix
    assert b.groups["attn_out"].producers == [f"{p}.self_attn.v_proj.weight", f"{p}.self_attn.v_proj.bias"]
    assert b.groups["attn_out"].foldable
    assert f"{p}.self_attn.v_proj.bias" in b.tensor_names()
    assert f"{p}.self_attn.q_proj.bias" not in b.tensor_names()       # added after the matmul: no fold
    sh = llama_shapes(layers=1)
    sh[f"{p}.mlp.up_proj.bias"] = (256,)
    (b,) = plan(sh, "qwen2")
    assert b.groups["mlp_out"].producers == [f"{p}.mlp.up_proj.weight", f"{p}.mlp.up_proj.bias"]


def test_plan_missing_norm_or_member():
    sh = llama_shapes(layers=1)
    del sh[f"{P}.0.post_attention_layernorm.weight"]
    (b,) = plan(sh)
    assert not b.groups["mlp_in"].foldable and "missing producer" in b.groups["mlp_in"].reason
    assert all(b.groups[n].foldable for n in ("attn_in", "attn_out", "mlp_out"))
    sh = llama_shapes(layers=1)
    del sh[f"{P}.0.self_attn.k_proj.weight"]
    (b,) = plan(sh)
    assert not b.groups["attn_in"].foldable and "missing member" in b.groups["attn_in"].reason
    assert b.groups["attn_in"].members == [f"{P}.0.self_attn.q_proj.weight", f"{P}.0.self_attn.v_proj.weight"]
    # a member the GEMM layout cannot hold (in_features % group_size) is not a member
    sh = llama_shapes(layers=1)
    (b,) = plan(sh, group_size=128)    # hidden 128, intermediate 256: all fine
    assert all(g.foldable for g in b.groups.values())
    sh[f"{P}.0.mlp.down_proj.weight"] = (128, 200)
    (b,) = plan(sh, group_size=128)
    assert "mlp_out" not in b.groups


def test_plan_rejects_other_model_types():
    for mt in ("opt", "gemma", "mixtral", "gpt2", None):
        with pytest.raises(ValueError, match="llama, mistral, qwen2"):
            plan(llama_shapes(layers=1), mt)
    assert len(plan(llama_shapes(layers=1), "mistral")) == 1


def test_plan_head_and_embeddings_in_no_group():
    sh = llama_shapes()
    sh["model.extra_proj.weight"] = (128, 128)          # a linear outside every block
    sh[f"{P}.1.self_attn.rotary.weight"] = (64, 128)    # a linear inside a block, in no group
    blocks = plan(sh)
    used = {n for b in blocks for n in b.tensor_names()}
    for n in ("lm_head.weight", "model.embed_tokens.weight", "model.norm.weight"):
        assert n not in used and n not in blocks.ungrouped
    assert blocks.ungrouped == ["model.extra_proj.weight", f"{P}.1.self_attn.rotary.weight"]


# ---------------------------------------------------------------- the flag
def _model_dir(tmp_path, model_type):
    d = tmp_path / f"model_{model_type}"
    d.mkdir()
    g = torch.Generator().manual_seed(0)
    save_file({n: torch.randn(s, generator=g).bfloat16() for n, s in llama_shapes(layers=1).items()},
              str(d / "model.safetensors"))
    with open(d / "config.json", "w") as f:
        json.dump({"model_type": model_type}, f)
    p = str(tmp_path / f"stats_{model_type}.safetensors")
    save_file({f"{P}.0.mlp.down_proj.weight.x_mean": torch.ones(256),
               f"{P}.0.mlp.down_proj.weight.x_sq": torch.ones(256)}, p)
    return str(d), p


def test_parse_args_accepts_fold_scales():
    from awq_quantizer.main import parse_args
    a = parse_args(["--model_id", "m", "--output_dir", "o", "--fold_scales"])
    assert a.fold_scales is True
    assert parse_args(["--model_id", "m", "--output_dir", "o"]).fold_scales is False


def test_main_fold_scales_needs_its_prerequisites(tmp_path, monkeypatch):
    from awq_quantizer.main import main
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    d, p = _model_dir(tmp_path, "llama")
    full = {"--scale_method": "awq", "--act_stats": p, "--output_format": "autoawq"}
    for drop in full:
        argv = ["--model_id", d, "--output_dir", str(tmp_path / "o"), "--device", "cpu", "--group_size", "32",
                "--log_level", "CRITICAL", "--fold_scales"]
        for k, v in full.items():
            if k != drop:
                argv += [k, v]
        assert main(argv) == 1, drop
        assert not os.path.exists(tmp_path / "o" / "model.safetensors")


def test_main_fold_scales_refuses_model_type_and_torchrun(tmp_path, monkeypatch, capsys):
    from awq_quantizer.main import main
    monkeypatch.delenv("WORLD_SIZE", raising=False)

    def run(d, p, out):
        return main(["--model_id", d, "--output_dir", str(tmp_path / out), "--device", "cpu", "--group_size", "32",
                     "--log_level", "ERROR", "--scale_method", "awq", "--act_stats", p, "--output_format", "autoawq",
                     "--fold_scales"])

    d, p = _model_dir(tmp_path, "opt")
    assert run(d, p, "o1") == 1
    assert "model types llama, mistral, qwen2" in capsys.readouterr().out   # (the CLI logs to stdout)
    d, p = _model_dir(tmp_path, "llama")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    assert run(d, p, "o2") == 1
    assert "torchrun" in capsys.readouterr().out


# ---------------------------------------------------------------- the library
def test_fold_rows_exported_and_checks_arguments_without_device():
    from awq_quantizer import _hip
    lib = _hip.load_library()
    assert hasattr(lib, "awq_fold_rows") and "awq_fold_rows" in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["awq_fold_rows"][1]) == 7
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL, EUNSUPPORTED = 1, 2
    for dt in (0, 1, 2):
        assert lib.awq_fold_rows(None, dt, 4, 8, p, p, None) == EINVAL
        assert lib.awq_fold_rows(p, dt, 4, 8, None, p, None) == EINVAL
        assert lib.awq_fold_rows(p, dt, 4, 8, p, None, None) == EINVAL
        assert b"null" in lib.awq_last_error()
        assert lib.awq_fold_rows(p, dt, -1, 8, p, p, None) == EINVAL
        assert lib.awq_fold_rows(p, dt, 4, -8, p, p, None) == EINVAL
        assert lib.awq_fold_rows(p, dt, 0, 8, p, p, None) == 0        # empty: nothing launched
        assert lib.awq_fold_rows(p, dt, 4, 0, p, p, None) == 0
        assert lib.awq_fold_rows(None, dt, 0, 8, None, None, None) == 0  # ... and the pointers not looked at
        assert lib.awq_last_error() == b""
        assert lib.awq_fold_rows(p, dt, 1 << 40, 1 << 40, p, p, None) == EINVAL     # rows * K wraps int64
        assert lib.awq_fold_rows(p, dt, 1 << 62, 4, p, p, None) == EINVAL           # ... to 0
        assert b"too large" in lib.awq_last_error()
    for dt in (3, 4, -1):                                             # fp64, integers
        assert lib.awq_fold_rows(p, dt, 4, 8, p, p, None) == EUNSUPPORTED
    assert lib.awq_abi_version() == 17                                # additive
    with pytest.raises(ValueError, match="bf16 / fp16 / fp32"):
        _hip.fold_rows(torch.zeros(4, 8, dtype=torch.float64), torch.ones(4))
    with pytest.raises(ValueError, match="row_scale"):
        _hip.fold_rows(torch.zeros(4, 8), torch.ones(3))


def test_rtn_warning_only_without_act_stats(tmp_path, monkeypatch, capsys):
    """"--scale_method awq without --act_stats" is said only when no statistics are given (with
    or without --act_clip).  Only the message is checked: without a GPU each run ends with 1 after
    the flags are checked, with one it goes on to quantize."""
    from awq_quantizer.main import main
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    d, p = _model_dir(tmp_path, "llama")
    base = ["--model_id", d, "--output_dir", str(tmp_path / "o"), "--device", "cpu", "--group_size", "32",
            "--log_level", "WARNING", "--scale_method", "awq", "--output_format", "packed"]
    main(base)
    assert "without --act_stats" in capsys.readouterr().out
    for extra in ([], ["--act_clip"]):
        main(base + ["--act_stats", p] + extra)
        assert "without --act_stats" not in capsys.readouterr().out
