"""--output_format gptq end to end on the three model fixtures (tests/golden/model_<arch>/): the CLI
writes every variant twice, as a GPTQ and as an AutoAWQ checkpoint with the same flags; the GPTQ
directory is read by tests/gptq_reader.py (the published formula, no awq_quantizer code), the
AutoAWQ one by tests/checkpoint_reader.py, and both go through tests/model_forward.py's float64
forward.  The two layouts hold the same fields and the same scale bits in another order, so

  * every weight either reader forms is the same float64 number, exactly (symmetric too: both
    readers subtract the stored zero field 8 from the field q + 8);
  * the logits are therefore equal: asserted exactly for the asymmetric variants; for the symmetric
    ones to float64 round-off, ||d||_F <= 1e-12 ||logits||_F (2^-53 per operation over a few thousand
    accumulated terms is ~1e-13; a single differing 4-bit field moves the logits by ~1e-4).

verify returns 0 on every GPTQ directory, and 1 once one g_idx entry or (symmetric) one stored zero
is altered; evaluate prints the same figures for a GPTQ directory as for its AutoAWQ twin.
Each CLI run is made once per module."""
import json
import shutil

import pytest
import torch
from safetensors.torch import load_file, save_file

import model_cases as mc
from checkpoint_reader import read_autoawq
from gptq_reader import read_gptq
from model_forward import model_forward

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]

VARIANTS = ("rtn", "rtn_sym", "fold", "fold_sym")
CASES = [(a, v) for a in mc.ARCHS for v in VARIANTS]
ASYM = [(a, v) for a, v in CASES if not v.endswith("_sym")]
FORMAT_OF = {"rtn": "gptq", "rtn_sym": "gptq_v2", "fold": "gptq_v2", "fold_sym": "gptq"}   # both formats, both modes


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from awq_quantizer import _hip
    from awq_quantizer.main import main
    _hip.require_device(torch.device("cuda", 0))
    models, done = {}, {}

    def model_dir(arch):
        if arch not in models:
            fx = mc.fixture(arch)
            d = tmp_path_factory.mktemp(f"gptq_{arch}")
            save_file({k: v.contiguous() for k, v in fx.state.items()}, str(d / "model.safetensors"),
                      metadata={"format": "pt"})
            with open(d / "config.json", "w") as f:
                json.dump(fx.config, f)
            save_file({"input_ids": fx.input_ids}, str(d) + "_ids.safetensors")
            models[arch] = str(d)
        return models[arch]

    def written(arch, variant, layout):
        key = (arch, variant, layout)
        if key not in done:
            fx = mc.fixture(arch)
            out = str(tmp_path_factory.mktemp(f"gptqout_{arch}_{variant}_{layout}"))
            argv = ["--model_id", model_dir(arch), "--output_dir", out, "--log_level", "ERROR", "--group_size", "32",
                    "--device", "cuda:0", "--output_format", layout]
            if layout == "gptq":
                argv += ["--gptq_format", FORMAT_OF[variant]]
            if variant.startswith("fold"):
                argv += ["--scale_method", "awq", "--act_stats", fx.stats_path, "--fold_scales"]
            if variant.endswith("_sym"):
                argv += ["--symmetric"]
            assert main(argv) == 0
            done[key] = out
        return done[key]

    class Env:
        pass
    e = Env()
    e.model_dir, e.written = model_dir, written
    return e


@pytest.mark.parametrize("arch,variant", CASES, ids=[f"{a}-{v}" for a, v in CASES])
def test_gptq_checkpoint_is_its_autoawq_twin(env, arch, variant):
    fx = mc.fixture(arch)
    out = env.written(arch, variant, "gptq")
    state, info = read_gptq(out)
    twin, twin_info = read_autoawq(env.written(arch, variant, "autoawq"))
    sym = variant.endswith("_sym")
    # the files
    qc = info["quantize_config"]
    want = {"quant_method": "gptq", "bits": 4, "group_size": 32, "sym": sym, "desc_act": False,
            "checkpoint_format": FORMAT_OF[variant]}
    assert {k: qc[k] for k in want} == want
    assert json.load(open(out + "/config.json"))["quantization_config"] == want
    assert {n: tuple(t.shape) for n, t in state.items()} == fx.names
    assert set(info["quantized"]) == set(fx.quantized_names("autoawq")) == set(twin_info["quantized"])
    for name, p in info["quantized"].items():
        N, K = fx.names[name]
        assert p["qweight"].shape == (K // 8, N) and p["qzeros"].shape == (K // 32, N // 8)
        assert p["scales"].shape == (K // 32, N) and p["scales"].dtype == torch.float16
        assert p["g_idx"].dtype == torch.int32 and p["g_idx"].tolist() == [k // 32 for k in range(K)]
        if sym:                                                      # stored zero: 8, or 7 under v1
            stored = (8 - (1 if FORMAT_OF[variant] == "gptq" else 0)) * 0x11111111
            assert bool((p["qzeros"] == (stored - (1 << 32) if stored >= 1 << 31 else stored)).all())
    if variant.startswith("fold"):
        a, b = load_file(out + "/awq_scales.safetensors"), load_file(env.written(arch, variant, "autoawq") +
                                                                     "/awq_scales.safetensors")
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    # the same weights, the same function
    assert set(state) == set(twin)
    for name in state:
        assert torch.equal(state[name], twin[name]), name
    logits = model_forward(state, fx.config, fx.input_ids)
    ref = model_forward(twin, fx.config, fx.input_ids)
    d = float((logits - ref).norm() / ref.norm())
    print(f"gptq vs autoawq {arch} {variant}: ||d||/||ref|| {d:.3e}  e vs the source {fx.e(state):.3e}")
    if sym:
        assert d <= 1e-12
    else:
        assert torch.equal(logits, ref)
    if not sym:                                                      # (the textbook reference is asymmetric)
        assert fx.e(state) < mc.THETA * mc.e_textbook(arch, "autoawq", 32)


def _verify(src, out):
    from awq_quantizer import verify
    return verify.main(["--model_id", src, "--quantized_dir", out, "--device", "cuda:0", "--log_level", "CRITICAL"])


@pytest.mark.parametrize("arch,variant", CASES, ids=[f"{a}-{v}" for a, v in CASES])
def test_verify_accepts_and_names_alterations(env, arch, variant, tmp_path):
    src, out = env.model_dir(arch), env.written(arch, variant, "gptq")
    assert _verify(src, out) == 0
    rep = json.load(open(out + "/quantization_error.json"))
    assert rep["layout"] == "gptq" and rep["problems"] == {} and rep["fold_audited"] == variant.startswith("fold")
    assert set(rep["tensors"]) == set(mc.fixture(arch).quantized_names("autoawq"))
    layer = "model.layers.1.mlp.down_proj"

    def altered(key, change):
        d = str(tmp_path / key.rpartition(".")[2])
        shutil.copytree(out, d)
        t = load_file(d + "/model.safetensors")
        t[key] = t[key].clone()
        change(t[key])
        save_file(t, d + "/model.safetensors", metadata={"format": "pt"})
        rc = _verify(src, d)
        return rc, json.load(open(d + "/quantization_error.json"))["problems"]

    def bump(g):
        g[40] = 0                                                    # one entry: 40 // 32 = 1
    rc, problems = altered(f"{layer}.g_idx", bump)
    assert rc == 1 and set(problems) == {f"{layer}.weight"} and "act-order" in problems[f"{layer}.weight"]
    if variant.endswith("_sym"):
        def flip(z):
            z[1, 3] ^= 1 << 20                                       # one stored zero
        rc, problems = altered(f"{layer}.qzeros", flip)
        assert rc == 1 and set(problems) == {f"{layer}.weight"} and "other than 8" in problems[f"{layer}.weight"]


@pytest.mark.parametrize("arch,variant", ASYM, ids=[f"{a}-{v}" for a, v in ASYM])
def test_evaluate_prints_the_twins_figures(env, arch, variant, capsys):
    from awq_quantizer import evaluate
    src = env.model_dir(arch)
    base = ["--model_id", src, "--input_ids", src + "_ids.safetensors", "--log_level", "ERROR", "--device", "cuda:0",
            "--compute_dtype", "float32"]
    lines = {}
    for layout in ("gptq", "autoawq"):
        assert evaluate.main(base + ["--quantized_dir", env.written(arch, variant, layout)]) == 0
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        lines[layout] = {k: v for k, v in line.items() if not isinstance(v, str)}
    assert lines["gptq"] == lines["autoawq"]
    assert lines["gptq"]["kl_mean"] > 0 and lines["gptq"]["n_tokens_scored"] == 46      # a quantized model was scored
