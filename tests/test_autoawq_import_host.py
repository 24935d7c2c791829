"""Reading AutoAWQ checkpoints back, the parts that need no GPU: the C call's refusals
(include/awq_hip.h awq_import_autoawq_gemm), import_autoawq's shape errors, verify's detection of an
--output_format autoawq directory and its quant_config.json, and the fold audit (verify.fold_audit)
on toy llama-shaped directories with torch's CPU fold, a CPU import (the oracle's unpack and
pack_rows) and a stubbed error function."""
import json

import pytest
import torch
from safetensors.torch import load_file, save_file

from oracle import awq_oracle as orc

GS = 32
L0 = "model.layers.0"


def _lib():
    from awq_quantizer import _hip
    return _hip.load_library()


# ---------------------------------------------------------------- the C call
def test_import_refusals_without_gpu():
    from awq_quantizer import _hip
    lib = _lib()
    one = 0x1000                                                     # never dereferenced: refused first
    assert lib.awq_import_autoawq_gemm(None, None, None, 64, 256, 128, 8, None, None, None, None) != 0
    assert "4-bit" in _hip.last_error()
    assert lib.awq_import_autoawq_gemm(None, None, None, 60, 256, 128, 4, one, None, None, None) != 0
    assert "% 8" in _hip.last_error()
    assert lib.awq_import_autoawq_gemm(None, None, None, 64, 200, 128, 4, one, None, None, None) != 0
    assert "group_size" in _hip.last_error() and "% 8" in _hip.last_error()
    assert lib.awq_import_autoawq_gemm(one, one, one, 64, 256, 128, 4, None, None, None, None) != 0
    assert "at least one output" in _hip.last_error()
    assert lib.awq_import_autoawq_gemm(None, one, one, 64, 256, 128, 4, one, None, None, None) != 0
    assert "without its input" in _hip.last_error()
    assert lib.awq_import_autoawq_gemm(one, one, one, 64, 256, 0, 4, one, one, one, None) != 0
    assert "Group size" in _hip.last_error()
    assert lib.awq_abi_version() == 17                               # additive


def test_import_autoawq_shape_errors():
    from awq_quantizer.quantization import AWQQuantizer
    q = AWQQuantizer(bits=4, group_size=128, symmetric=False, device="cpu", logger_level="ERROR")
    ok = {"qweight": torch.zeros((256, 8), dtype=torch.int32), "qzeros": torch.zeros((2, 8), dtype=torch.int32),
          "scales": torch.zeros((2, 64), dtype=torch.float16)}
    for key, bad in (("qweight", torch.zeros((256, 9), dtype=torch.int32)),
                     ("qzeros", torch.zeros((3, 8), dtype=torch.int32)),
                     ("scales", torch.zeros((2, 72), dtype=torch.float16)),
                     ("scales", torch.zeros(128, dtype=torch.float16))):
        with pytest.raises(ValueError, match=key):
            q.import_autoawq(dict(ok, **{key: bad}))
    with pytest.raises(ValueError, match="scales"):
        q.import_autoawq({k: v for k, v in ok.items() if k != "scales"})
    with pytest.raises(ValueError, match="group_size"):
        q.import_autoawq(ok, group_size=96)                          # 256 % 96 != 0
    with pytest.raises(ValueError, match="qzeros"):
        q.import_autoawq(ok, group_size=64)                          # G = 4, qzeros has 2 rows


# ---------------------------------------------------------------- toy directories
def cpu_fold(w, s):
    """torch's CPU expression of fold_rows: an fp32 division, one rounding into the dtype."""
    return (w.float() / s.float().reshape([-1] + [1] * (w.dim() - 1))).to(w.dtype)


def cpu_import(gemm, group_size, symmetric):
    """import_autoawq restated on the CPU: the oracle's unpack, then its row-major pack."""
    iw, zz = orc.autoawq_unpack(gemm["qweight"], gemm["qzeros"])
    K, N = iw.shape
    return {"qweight": orc.pack_rows(iw.t().contiguous().to(torch.int32), 4, 0),
            "qzeros": orc.pack_rows(zz.t().contiguous().to(torch.int32), 4, 0),
            "scales": gemm["scales"].t().contiguous(), "bits": torch.tensor(4, dtype=torch.int32),
            "group_size": torch.tensor(group_size, dtype=torch.int32),
            "symmetric": torch.tensor(symmetric, dtype=torch.bool), "shape": torch.tensor([N, K], dtype=torch.int64)}


def source_tensors():
    g = torch.Generator().manual_seed(3)
    mk = lambda *sh: (torch.randn(*sh, generator=g) * 0.05).bfloat16()
    t = {"model.embed_tokens.weight": mk(64, 128), "model.norm.weight": torch.ones(128).bfloat16(),
         "lm_head.weight": mk(64, 128)}
    for p in (L0, "model.layers.1"):
        t.update({f"{p}.input_layernorm.weight": (1 + 0.1 * torch.randn(128, generator=g)).bfloat16(),
                  f"{p}.post_attention_layernorm.weight": (1 + 0.1 * torch.randn(128, generator=g)).bfloat16(),
                  f"{p}.self_attn.q_proj.weight": mk(128, 128), f"{p}.self_attn.k_proj.weight": mk(128, 128),
                  f"{p}.self_attn.v_proj.weight": mk(128, 128), f"{p}.self_attn.v_proj.bias": mk(128),
                  f"{p}.self_attn.o_proj.weight": mk(128, 128), f"{p}.mlp.gate_proj.weight": mk(256, 128),
                  f"{p}.mlp.up_proj.weight": mk(256, 128), f"{p}.mlp.down_proj.weight": mk(128, 256)})
    return t


def write_dirs(tmp_path, fold=True, model_type="llama", sidecar=True, ones=False):
    """(source dir, checkpoint dir, source tensors, sidecar): the checkpoint a --fold_scales run
    of block_plan's llama layout would leave — every linear a GEMM triple of random fields, norm
    weights and the v_proj bias folded with cpu_fold, everything else the source's."""
    from awq_quantizer.quantization.block_plan import plan_blocks
    src, out = tmp_path / "src", tmp_path / "out"
    src.mkdir()
    out.mkdir()
    tensors = source_tensors()
    save_file(tensors, str(src / "model.safetensors"))
    with open(src / "config.json", "w") as f:
        json.dump({"model_type": model_type}, f)
    g = torch.Generator().manual_seed(9)
    scale = lambda n: torch.ones(n) if ones else (0.5 + torch.rand(n, generator=g))
    ckpt, side = dict(tensors), {}
    plan = plan_blocks({n: tuple(t.shape) for n, t in tensors.items()}, "llama", GS)
    for block in plan:
        for gname in ("attn_out", "mlp_out", "attn_in", "mlp_in"):
            grp = block.groups[gname]
            assert grp.foldable
            s = scale(tensors[grp.members[0]].shape[1])
            for m in grp.members:
                side[f"{m}.input_scale"] = s.clone()
            if not fold:
                continue
            if grp.fold == "rows":
                side[f"{grp.producers[0]}.row_scale"] = s.clone()
                for pb in grp.producers[1:]:
                    ckpt[pb] = cpu_fold(tensors[pb], s)
            else:
                ckpt[grp.producers[0]] = cpu_fold(tensors[grp.producers[0]], s)
        for m in block.members():
            N, K = tensors[m].shape
            qw, qz, sc = orc.autoawq_pack(torch.randint(0, 16, (N, K), generator=g),
                                          torch.randint(0, 16, (N, K // GS), generator=g),
                                          torch.rand(N, K // GS, generator=g).half())
            del ckpt[m]
            ckpt.update({m[:-len("weight")] + "qweight": qw, m[:-len("weight")] + "qzeros": qz,
                         m[:-len("weight")] + "scales": sc})
    save_file(ckpt, str(out / "model.safetensors"))
    if sidecar:
        save_file(side, str(out / "awq_scales.safetensors"))
    with open(out / "quant_config.json", "w") as f:
        json.dump({"zero_point": True, "q_group_size": GS, "w_bit": 4, "version": "GEMM"}, f)
    return str(src), str(out), tensors, side


def run_verify(src, out):
    from awq_quantizer import verify
    from awq_quantizer.quantization.awq import error_report

    def stub(tensor, result):
        n = tensor.numel()
        return error_report(n, [n * 0.5, n * 0.25, n * 4.0, 0.75, 0.0])

    args = verify.parse_args(["--model_id", src, "--quantized_dir", out, "--log_level", "CRITICAL"])
    rc = verify.verify(args, error_fn=stub, import_fn=cpu_import, fold_fn=cpu_fold)
    return rc, json.load(open(f"{out}/quantization_error.json"))


def rewrite(path, change):
    t = load_file(path)
    change(t)
    save_file(t, path)


# ---------------------------------------------------------------- detection and settings
def test_directory_detection_and_quant_config(tmp_path):
    from awq_quantizer import verify
    src, out, tensors, _ = write_dirs(tmp_path)
    assert verify.is_autoawq_dir(out) and not verify.is_autoawq_dir(src + "/nothing")
    assert verify.autoawq_files(out) == [out + "/model.safetensors"]
    cfg, problems = verify.read_quant_config(out)
    assert cfg == {"group_size": GS, "symmetric": False, "not_converted": []} and problems == {}
    # a sharded directory: the index names the shards
    sh = tmp_path / "sharded"
    sh.mkdir()
    with open(sh / "model.safetensors.index.json", "w") as f:
        json.dump({"metadata": {}, "weight_map": {"a": "model-00002-of-00002.safetensors",
                                                  "b": "model-00001-of-00002.safetensors", "c": "model-00001-of-00002.safetensors"}}, f)
    assert verify.is_autoawq_dir(str(sh))
    assert verify.autoawq_files(str(sh)) == [str(sh / "model-00001-of-00002.safetensors"),
                                             str(sh / "model-00002-of-00002.safetensors")]
    # metadata.json marks the private formats
    (sh / "metadata.json").write_text("{}")
    assert not verify.is_autoawq_dir(str(sh))
    # settings: symmetric, modules_to_not_convert, and what is refused
    with open(f"{out}/quant_config.json", "w") as f:
        json.dump({"zero_point": False, "q_group_size": 64, "w_bit": 4, "modules_to_not_convert": ["x.y"]}, f)
    assert verify.read_quant_config(out) == ({"group_size": 64, "symmetric": True, "not_converted": ["x.y"]}, {})
    with open(f"{out}/quant_config.json", "w") as f:
        json.dump({"zero_point": True, "q_group_size": GS, "w_bit": 8}, f)
    assert set(verify.read_quant_config(out)[1]) == {"quant_config.json"}
    rc, rep = run_verify(src, out)
    assert rc == 1 and set(rep["problems"]) == {"quant_config.json"} and rep["tensors"] == {}
    (tmp_path / "out" / "quant_config.json").unlink()
    rc, rep = run_verify(src, out)
    assert rc == 1 and set(rep["problems"]) == {"quant_config.json"}


# ---------------------------------------------------------------- the report and the audit
def test_clean_directory_verifies_and_rebuilds_each_domain(tmp_path):
    src, out, tensors, side = write_dirs(tmp_path)
    rc, rep = run_verify(src, out)
    assert rc == 0 and rep["problems"] == {} and rep["skipped"] == {}
    linears = {n for n in tensors if n.endswith("_proj.weight")}
    assert set(rep["tensors"]) == linears and len(linears) == 14
    assert rep["layout"] == "autoawq" and rep["fold_audited"] is True
    assert set(rep["copied"]) == set(tensors) - linears
    for name, e in rep["tensors"].items():
        assert e["layout"] == "autoawq" and e["input_scaled"] is True
        assert e["row_folded"] == (name.endswith("v_proj.weight") or name.endswith("up_proj.weight")), name
    assert rep["totals"]["tensors"] == 14
    # the domain: fold_rows first, then input_scale handed to the error function
    from awq_quantizer import verify
    from awq_quantizer.quantization.awq import error_report
    got = {}

    def stub(tensor, result):
        got[tuple(result["qweight"].shape) + (len(got),)] = (tensor, result)
        return error_report(tensor.numel(), [1.0, 1.0, 4.0, 1.0, 0.0])

    args = verify.parse_args(["--model_id", src, "--quantized_dir", out, "--log_level", "CRITICAL"])
    assert verify.verify(args, error_fn=stub, import_fn=cpu_import, fold_fn=cpu_fold) == 0
    ck = load_file(out + "/model.safetensors")
    by_words = {}
    for tensor, result in got.values():
        by_words.setdefault(result["qweight"].numpy().tobytes(), []).append((tensor, result))
    for name in (f"{L0}.self_attn.v_proj.weight", f"{L0}.self_attn.q_proj.weight", f"{L0}.mlp.down_proj.weight"):
        want = cpu_import({k: ck[name[:-len("weight")] + k] for k in ("qweight", "qzeros", "scales")}, GS, False)
        (tensor, result), = by_words[want["qweight"].numpy().tobytes()]
        src_w = tensors[name]
        if f"{name}.row_scale" in side:
            src_w = cpu_fold(src_w, side[f"{name}.row_scale"])
        assert torch.equal(tensor.view(torch.int16), src_w.view(torch.int16)), name
        assert torch.equal(result["input_scale"], side[f"{name}.input_scale"]), name
        assert torch.equal(result["qzeros"], want["qzeros"]) and torch.equal(result["scales"], want["scales"])
        assert int(result["group_size"]) == GS and not bool(result["symmetric"])
    assert f"{L0}.self_attn.v_proj.weight.row_scale" in side and f"{L0}.self_attn.q_proj.weight.row_scale" not in side


def test_unfolded_norm_is_named(tmp_path):
    src, out, tensors, _ = write_dirs(tmp_path)
    norm = f"{L0}.input_layernorm.weight"
    rewrite(out + "/model.safetensors", lambda t: t.__setitem__(norm, tensors[norm].clone()))
    rc, rep = run_verify(src, out)
    assert rc == 1 and set(rep["problems"]) == {norm}
    assert f"{L0}:attn_in" in rep["problems"][norm]
    assert len(rep["tensors"]) == 14                                 # the report itself is still complete


def test_unfolded_bias_is_named(tmp_path):
    src, out, tensors, _ = write_dirs(tmp_path)
    bias = "model.layers.1.self_attn.v_proj.bias"
    rewrite(out + "/model.safetensors", lambda t: t.__setitem__(bias, tensors[bias].clone()))
    rc, rep = run_verify(src, out)
    assert rc == 1 and set(rep["problems"]) == {bias} and "model.layers.1:attn_out" in rep["problems"][bias]


def test_members_of_a_group_with_different_scales(tmp_path):
    src, out, tensors, side = write_dirs(tmp_path)
    key = f"{L0}.self_attn.k_proj.weight.input_scale"
    rewrite(out + "/awq_scales.safetensors", lambda t: t.__setitem__(key, side[key] * 2))
    rc, rep = run_verify(src, out)
    assert rc == 1 and set(rep["problems"]) == {key} and f"{L0}:attn_in" in rep["problems"][key]


def test_altered_copied_tensor(tmp_path):
    src, out, tensors, _ = write_dirs(tmp_path)
    name = "model.embed_tokens.weight"

    def flip(t):
        t[name] = t[name].clone()
        t[name].view(torch.int16)[5, 7] ^= 1                         # one bit
    rewrite(out + "/model.safetensors", flip)
    rc, rep = run_verify(src, out)
    assert rc == 1 and set(rep["problems"]) == {name} and name in rep["copied"]


def test_group_without_sidecar_scale_must_keep_the_source(tmp_path):
    """No scale for a group in the sidecar: its norm must be the source's (here it is folded)."""
    src, out, tensors, side = write_dirs(tmp_path)

    def drop(t):
        for n in ("q", "k", "v"):
            del t[f"{L0}.self_attn.{n}_proj.weight.input_scale"]
    rewrite(out + "/awq_scales.safetensors", drop)
    rc, rep = run_verify(src, out)
    assert rc == 1 and set(rep["problems"]) == {f"{L0}.input_layernorm.weight"}
    assert rep["tensors"][f"{L0}.self_attn.q_proj.weight"]["input_scaled"] is False


def test_plan_refusal_with_a_sidecar_is_one_problem(tmp_path):
    src, out, tensors, _ = write_dirs(tmp_path, model_type="opt", ones=True)
    rc, rep = run_verify(src, out)
    assert rc == 1 and set(rep["problems"]) == {"awq_scales.safetensors"}
    assert "opt" in rep["problems"]["awq_scales.safetensors"]


def test_plain_autoawq_directory_has_no_audit(tmp_path):
    src, out, tensors, _ = write_dirs(tmp_path, fold=False, sidecar=False)
    rc, rep = run_verify(src, out)
    assert rc == 0 and rep["problems"] == {} and rep["fold_audited"] is False
    assert all(e["input_scaled"] is False and e["row_folded"] is False for e in rep["tensors"].values())


def test_fold_audit_function_alone():
    """fold_audit on dictionaries: no files, no loader."""
    from awq_quantizer import verify
    tensors = source_tensors()
    shapes = {n: tuple(t.shape) for n, t in tensors.items()}
    s = 0.5 + torch.rand(128, generator=torch.Generator().manual_seed(1))
    side = {f"{L0}.self_attn.{n}_proj.weight.input_scale": s for n in "qkv"}
    norm = f"{L0}.input_layernorm.weight"
    ckpt = dict(tensors)
    ckpt[norm] = cpu_fold(tensors[norm], s)
    audit = lambda c, sd, mt="llama": verify.fold_audit(shapes, mt, GS, sd, tensors.__getitem__, c.get, cpu_fold)
    assert audit(ckpt, side) == {}
    assert set(audit(tensors, side)) == {norm}
    assert set(audit(ckpt, {})) == {norm}
    assert set(audit(ckpt, side, "gemma")) == {"awq_scales.safetensors"}
    assert set(audit({k: v for k, v in ckpt.items() if k != norm}, side)) == {norm}
    rows = dict(side, **{f"{L0}.self_attn.v_proj.weight.row_scale": s,
                         f"{L0}.self_attn.o_proj.weight.input_scale": s * 3})
    ck2 = dict(ckpt, **{f"{L0}.self_attn.v_proj.bias": cpu_fold(tensors[f"{L0}.self_attn.v_proj.bias"], s)})
    assert set(audit(ck2, rows)) == {f"{L0}.self_attn.v_proj.weight.row_scale"}
