"""Written checkpoints against an independent full-model forward.

Every case is one in-process CLI run on a tiny model directory (tests/golden/model_<arch>/ written
in the case's dtype: real Llama / Mistral (GQA) / Qwen2 (qkv bias) shapes and names, recorded from
transformers).  The output directory is read by tests/checkpoint_reader.py (plain integer ops, no
awq_quantizer code), pushed through tests/model_forward.py (float64, pinned to transformers by
tests/test_model_forward_host.py) on the fixture's input_ids, and
e = ||logits - ref||_F / ||ref||_F is taken against the recorded float64 logits.

  1. loadable: names and shapes are the source model's (names.json), and — when transformers is
     importable — a strict load_state_dict into the real class succeeds and the written config.json parses;
  2. reader vs. library: every quantized tensor as the reader forms it in float64 against
     AWQQuantizer.dequantize_autoawq / dequantize_packed, |d| <= 2^-11 |W| + 2^-25 (q - z is exact in
     fp16, the product is rounded once to fp16);
  3. function: e < THETA * e_textbook, the float64 textbook RTN of the same tensors at the same group
     size (model_cases.e_textbook; never the code under test); a reader with the identity nibble order
     or with every zero point + 1 exceeds that bound on the same files;
  4. --fold_scales is an equivalence of the whole model: the unquantized counterpart (W_src *
     diag(input_scale) / row_scale in float64 from awq_scales.safetensors, folded norm weights and
     biases as written) has e <= 3e-6 (fp32 directory) / n 2^-9 (bf16; n = the 4 norm weights, 6 with
     qwen2's v_proj biases, that are written rounded: model_cases.fold_bound, never above 2^-6); one
     source norm kept, every mlp_out fold inverted or the v_proj.bias folds dropped exceed it; and
     the plan: no attn_out fold with GQA (mistral), v_proj.bias folded (qwen2), v_proj row scales;
  5. the activation-aware checkpoints stay below THETA * e_textbook as well, and below the RTN
     checkpoint's e (measured e_awq / e_rtn 0.60 .. 0.75, more than the 1.2x that makes it an assertion).

Measured on an MI355X (THETA = 2.6; mutation columns are e_mut / e_textbook):
  RTN autoawq          e          e/e_textbook  identity nibble order  zero point + 1
  llama   bf16 gs32    6.107e-03  0.988         10.64                  17.81
  llama   fp16 gs32    6.163e-03  0.997         10.64                  17.52
  llama   fp32 gs32    6.198e-03  1.003         10.63                  17.47
  llama   bf16 gs64    7.030e-03  0.985          9.13                  26.10
  mistral bf16 gs32    6.155e-03  1.004         10.32                  14.15
  qwen2   bf16 gs32    7.152e-03  1.010         14.58                   7.23
  RTN packed bf16 gs32 (every tensor): llama 2.889e-01 (1.009), mistral 2.239e-01 (0.996), qwen2 2.869e-01 (0.997)

  --fold_scales gs32   counterpart e       source norm  mlp_out    v bias    e/e_textbook            e_awq/e_rtn
                       bf16      fp32      kept         inverted   dropped   search      +act_clip
  llama                1.335e-04 2.117e-09 5.550e-02    1.527e-02            0.739/0.742 0.712/0.712  0.71 .. 0.75
  mistral              1.109e-04 1.994e-09 4.913e-02    1.932e-02            0.692/0.706 0.688/0.673  0.67 .. 0.70
  qwen2                1.471e-04 2.156e-09 3.770e-02    1.598e-02  5.249e-02 0.648/0.664 0.610/0.604  0.60 .. 0.66
  (e/e_textbook: bf16/fp32 directory.  llama's inverted mlp_out fold, 1.527e-02, is under 2^-6 = 1.5625e-02:
  the reason the bf16 bound counts the tensors that are actually rounded.)
"""
import json
import os

import pytest
import torch
from safetensors.torch import load_file, save_file

import model_cases as mc
from checkpoint_reader import IDENTITY, read_autoawq, read_checkpoint

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
RTN_AUTOAWQ = [("llama", "bf16", 32), ("llama", "fp16", 32), ("llama", "fp32", 32), ("llama", "bf16", 64),
               ("mistral", "bf16", 32), ("qwen2", "bf16", 32)]
FOLD = [(a, d, c) for a in mc.ARCHS for d in ("bf16", "fp32") for c in (False, True)]


def _dev():
    from awq_quantizer import _hip
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    return dev


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """run(arch, dtype, variant, group_size) -> the case's record, each CLI run made once."""
    from awq_quantizer.main import main
    _dev()
    models, done = {}, {}

    def model_dir(arch, dtype):
        if (arch, dtype) not in models:
            fx = mc.fixture(arch)
            d = tmp_path_factory.mktemp(f"{arch}_{dtype}")
            save_file({k: v.to(DTYPES[dtype]) for k, v in fx.state.items()}, str(d / "model.safetensors"),
                      metadata={"format": "pt"})
            with open(d / "config.json", "w") as f:
                json.dump(fx.config, f)
            models[arch, dtype] = str(d)
        return models[arch, dtype]

    def run(arch, dtype, variant, group_size=32):
        key = (arch, dtype, variant, group_size)
        if key not in done:
            fx = mc.fixture(arch)
            out = str(tmp_path_factory.mktemp(f"out_{arch}_{dtype}_{variant}_{group_size}"))
            argv = ["--model_id", model_dir(arch, dtype), "--output_dir", out, "--log_level", "ERROR",
                    "--group_size", str(group_size), "--device", "cuda:0"]
            if variant == "packed":
                argv += ["--output_format", "packed", "--save_safetensors"]
            elif variant == "autoawq":
                argv += ["--output_format", "autoawq"]
            else:
                argv += ["--output_format", "autoawq", "--scale_method", "awq", "--act_stats", fx.stats_path,
                         "--fold_scales"] + (["--act_clip"] if variant == "fold_clip" else [])
            assert main(argv) == 0
            state, info = read_checkpoint(out)
            done[key] = {"out": out, "state": state, "info": info, "e": fx.e(state)}
        return done[key]

    return run


def check_loadable(fx, rec):
    state = rec["state"]
    assert {n: tuple(t.shape) for n, t in state.items()} == fx.names
    fmt = rec["info"]["format"]
    assert set(rec["info"]["quantized"]) == set(fx.quantized_names(fmt))
    try:
        import transformers
    except ImportError:
        return
    if fmt == "autoawq":
        cfg = transformers.AutoConfig.from_pretrained(rec["out"])
        qc = cfg.quantization_config if isinstance(cfg.quantization_config, dict) else cfg.quantization_config.to_dict()
        assert (qc["quant_method"], qc["bits"], qc["group_size"]) == ("awq", 4, rec["info"]["group_size"])
        assert "modules_to_not_convert" not in qc
        cfg = type(cfg).from_dict({k: v for k, v in cfg.to_dict().items() if k != "quantization_config"})
    else:
        cfg = transformers.AutoConfig.for_model(**fx.config)
    cls = {"llama": transformers.LlamaForCausalLM, "mistral": transformers.MistralForCausalLM,
           "qwen2": transformers.Qwen2ForCausalLM}[fx.arch]
    model = cls(cfg)
    model.load_state_dict({k: v.float() for k, v in state.items()}, strict=True)


def check_reader_against_library(rec, group_size):
    from awq_quantizer.quantization.awq import AWQQuantizer
    q = AWQQuantizer(bits=4, group_size=group_size, symmetric=False, device="cuda:0", logger_level="ERROR")
    dev = _dev()
    for name, parts in rec["info"]["quantized"].items():
        if rec["info"]["format"] == "autoawq":
            lib = q.dequantize_autoawq(parts, group_size=group_size, symmetric=False)
        else:
            lib = q.dequantize_packed({k: (v.to(dev) if k in ("qweight", "qzeros", "scales") else v)
                                       for k, v in parts.items()})
        lib = lib.cpu().double().reshape(rec["state"][name].shape)
        w = rec["state"][name]
        assert bool(((lib - w).abs() <= 2.0 ** -11 * w.abs() + 2.0 ** -25).all()), name


@pytest.mark.parametrize("arch,dtype,group_size", RTN_AUTOAWQ,
                         ids=[f"{a}-{d}-gs{g}" for a, d, g in RTN_AUTOAWQ])
def test_rtn_autoawq_checkpoint(runs, arch, dtype, group_size):
    fx = mc.fixture(arch)
    rec = runs(arch, dtype, "autoawq", group_size)
    check_loadable(fx, rec)
    check_reader_against_library(rec, group_size)
    if group_size == 64:                       # G = 2: one qzeros word per 8 columns, rows of scales [2, N]
        assert rec["info"]["quantized"]["model.layers.0.self_attn.q_proj.weight"]["qzeros"].shape == (2, 16)
    et = mc.e_textbook(arch, "autoawq", group_size)
    wrong = {"identity_nibble_order": fx.e(read_autoawq(rec["out"], order=IDENTITY)[0]),
             "zero_point_plus_1": fx.e(read_autoawq(rec["out"], zero_shift=1)[0])}
    print(f"rtn autoawq {arch} {dtype} gs{group_size}: e {rec['e']:.3e}  e/e_textbook {rec['e'] / et:.3f}  " +
          "  ".join(f"{k} {v / et:.2f}" for k, v in wrong.items()))
    assert rec["e"] < mc.THETA * et
    for label, e in wrong.items():
        assert e > mc.THETA * et, label


@pytest.mark.parametrize("arch", mc.ARCHS)
def test_rtn_packed_checkpoint(runs, arch):
    """--output_format packed quantizes every tensor of >= 128 elements (norms, biases, embeddings
    and lm_head too), so the textbook reference does the same."""
    fx = mc.fixture(arch)
    rec = runs(arch, "bf16", "packed")
    check_loadable(fx, rec)
    check_reader_against_library(rec, 32)
    et = mc.e_textbook(arch, "packed", 32)
    print(f"rtn packed {arch} bf16 gs32: e {rec['e']:.3e}  e/e_textbook {rec['e'] / et:.3f}")
    assert rec["e"] < mc.THETA * et


@pytest.mark.parametrize("arch,dtype,clip", FOLD,
                         ids=[f"{a}-{d}-{'act_clip' if c else 'search'}" for a, d, c in FOLD])
def test_fold_scales_checkpoint(runs, arch, dtype, clip):
    fx = mc.fixture(arch)
    rec = runs(arch, dtype, "fold_clip" if clip else "fold")
    check_loadable(fx, rec)
    check_reader_against_library(rec, 32)
    scales = load_file(os.path.join(rec["out"], "awq_scales.safetensors"))
    written = {n: t for n, t in rec["state"].items() if n not in rec["info"]["quantized"]}

    # the plan
    L = "model.layers"
    assert {k[: -len(".input_scale")] for k in scales if k.endswith(".input_scale")} == set(
        fx.quantized_names("autoawq"))
    for i in range(fx.layers):
        v_rows, up_rows = f"{L}.{i}.self_attn.v_proj.weight.row_scale", f"{L}.{i}.mlp.up_proj.weight.row_scale"
        o_in = scales[f"{L}.{i}.self_attn.o_proj.weight.input_scale"]
        assert up_rows in scales and torch.equal(scales[up_rows], scales[f"{L}.{i}.mlp.down_proj.weight.input_scale"])
        if arch == "mistral":                 # GQA: 64 v_proj rows for 128 o_proj inputs, no one-to-one fold
            assert v_rows not in scales and torch.equal(o_in, torch.ones_like(o_in))
        else:
            assert torch.equal(scales[v_rows], o_in) and not torch.equal(o_in, torch.ones_like(o_in))
        for m in ("q", "k", "v"):
            assert torch.equal(scales[f"{L}.{i}.self_attn.{m}_proj.weight.input_scale"],
                               scales[f"{L}.{i}.self_attn.q_proj.weight.input_scale"])
        assert torch.equal(scales[f"{L}.{i}.mlp.gate_proj.weight.input_scale"],
                           scales[f"{L}.{i}.mlp.up_proj.weight.input_scale"])
        for norm in ("input_layernorm", "post_attention_layernorm"):
            assert not torch.equal(written[f"{L}.{i}.{norm}.weight"], fx.source[f"{L}.{i}.{norm}.weight"])
        if arch == "qwen2":
            vb = f"{L}.{i}.self_attn.v_proj.bias"
            want = (fx.source[vb].float() / scales[v_rows]).to(DTYPES[dtype]).double()
            assert torch.equal(written[vb], want) and not torch.equal(written[vb], fx.source[vb])
            for m in ("q", "k"):
                assert torch.equal(written[f"{L}.{i}.self_attn.{m}_proj.bias"], fx.source[f"{L}.{i}.self_attn.{m}_proj.bias"])
    changed = {n for n in written if not torch.equal(written[n], fx.source[n])}
    assert changed == {n for n in written if "layernorm" in n or n.endswith("v_proj.bias")}

    # the fold is an equivalence of the whole model
    bound = mc.fold_bound(fx, DTYPES[dtype])
    es = {k: fx.e(s) for k, s in mc.fold_mutations(fx, scales, written).items()}
    print(f"fold {arch} {dtype} {'act_clip' if clip else 'search'}: " + "  ".join(f"{k} {v:.3e}" for k, v in es.items()))
    assert set(es) == {"none", "source_norm_kept", "mlp_out_fold_inverted"} | (
        {"v_bias_fold_dropped"} if arch == "qwen2" else set())
    assert es.pop("none") <= bound
    for label, e in es.items():
        assert e > bound, label

    # the quantized function
    et = mc.e_textbook(arch, "autoawq", 32)
    e_rtn = runs(arch, dtype if dtype != "fp32" or arch == "llama" else "bf16", "autoawq")["e"]
    print(f"fold {arch} {dtype} {'act_clip' if clip else 'search'}: e {rec['e']:.3e}  e/e_textbook "
          f"{rec['e'] / et:.3f}  e_awq/e_rtn {rec['e'] / e_rtn:.3f}")
    assert rec["e"] < mc.THETA * et
    assert rec["e"] <= e_rtn                   # measured 0.60 .. 0.74: more than the 1.2x that makes it an assertion
