"""The measuring instruments of tests/test_gpu_model_forward.py, checked on the CPU:

  1. tests/model_forward.py equals the float64 logits recorded from transformers' own Llama,
     Mistral and Qwen2 classes (tests/golden/model_<arch>/) to 1e-9 max|logits|;
  2. with transformers importable: the fixtures are not stale (the real classes reproduce the
     recorded logits), and the config.json that write_autoawq_configs writes parses;
  3. the checks can fail: a textbook float64 RTN of every block linear, packed into the published
     GEMM layout, then read back with the identity nibble order or with every zero point + 1, and a
     host-made fold with one source norm kept, the mlp_out fold inverted or the v_proj.bias fold
     dropped — each exceeds the bound of the assertion it targets.

Measured (e = ||logits - ref||_F / ||ref||_F; ratios are e_mut / e_textbook):

  arch     gs  e_textbook  identity nibble order  zero point + 1
  llama    32  6.181e-03   10.63                  17.46
  llama    64  7.135e-03    9.13                  25.83
  mistral  32  6.130e-03   10.36                  14.09
  mistral  64  6.832e-03    9.21                  20.90
  qwen2    32  7.084e-03   14.51                   7.19
  qwen2    64  8.210e-03   12.71                   9.64
  smallest ratio 7.19 -> THETA = 2.6 <= sqrt(7.19) = 2.68 (model_cases.THETA)

  host fold (s = sqrt(x_mean), normalised)   fp32 dir    bf16 dir    bound 3e-6 / n 2^-9 (7.8e-3; qwen2 1.17e-2)
  llama    none                              1.71e-09    8.68e-05
           source norm kept                  8.49e-02    8.49e-02
           mlp_out fold inverted             3.03e-02    3.03e-02
  mistral  none                              1.55e-09    8.55e-05
           source norm kept                  7.21e-02    7.21e-02
           mlp_out fold inverted             3.14e-02    3.14e-02
  qwen2    none                              1.82e-09    1.26e-04
           source norm kept                  5.92e-02    5.92e-02
           mlp_out fold inverted             2.36e-02    2.36e-02
           v_proj.bias fold dropped          9.37e-02    9.37e-02
"""
import argparse
import importlib.util
import json
import os

import pytest
import torch

import model_cases as mc
from checkpoint_reader import dequant_gemm, dequant_packed
from model_forward import model_forward

ARCHS = mc.ARCHS


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_model",
                                                  os.path.join(mc.GOLDEN, "make_golden_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("arch", ARCHS)
def test_plain_forward_equals_recorded_logits(arch):
    fx = mc.fixture(arch)
    assert set(fx.state) == set(fx.names) and all(tuple(fx.state[n].shape) == s for n, s in fx.names.items())
    got = model_forward(fx.source, fx.config, fx.input_ids)
    err = float((got - fx.logits).abs().max())
    print(f"{arch}: max |plain forward - recorded| = {err:.3e}, max|logits| = {float(fx.logits.abs().max()):.4f}")
    assert fx.logits.dtype == torch.float64 and tuple(fx.logits.shape) == (2, 24, 256)
    assert err <= 1e-9 * float(fx.logits.abs().max())


@pytest.mark.parametrize("arch", ARCHS)
def test_fixture_values_are_exact_in_every_dtype(arch):
    fx = mc.fixture(arch)
    for name, t in fx.state.items():
        assert t.dtype == torch.bfloat16
        assert torch.equal(t.double(), t.half().double()), name            # exact in fp16 too
    assert os.path.getsize(os.path.join(fx.dir, "model.safetensors")) < 1_000_000
    linears = [n for n in fx.names if len(fx.names[n]) == 2 and "embed" not in n]
    assert {n + s for n in linears for s in (".x_mean", ".x_sq")} == set(fx.stats)


@pytest.mark.parametrize("arch", ARCHS)
def test_fixture_is_what_transformers_computes(arch):
    """Not stale: the real class, loaded strictly, reproduces the recorded logits — in float64
    throughout to the bound of test 1, and as transformers stands (its RoPE angles, RMSNorm variance
    and softmax stay fp32: 9 such roundings of 2^-24 on the path, a few units of amplification each)
    to 2e-6 max|logits| (measured 1.1e-7), so the float64 replacements changed nothing but precision."""
    pytest.importorskip("transformers")
    gen = _generator()
    fx = mc.fixture(arch)
    cls, config = gen.model_class_and_config(arch)
    with open(os.path.join(fx.dir, "config.json")) as f:
        recorded, now = json.load(f), json.loads(json.dumps(config.to_dict()))
    assert {**recorded, "transformers_version": None} == {**now, "transformers_version": None}
    top = float(fx.logits.abs().max())
    for stock, bound in ((False, 1e-9), (True, 2e-6)):
        model = gen.float64_model(cls, config, fx.state, stock=stock)
        with torch.no_grad():
            got = model(input_ids=fx.input_ids).logits
        err = float((got - fx.logits).abs().max())
        print(f"{arch}: transformers ({'stock' if stock else 'float64'}) vs fixture: {err:.3e}")
        assert got.dtype == torch.float64 and err <= bound * top
    stats = gen.linear_input_stats(gen.float64_model(cls, config, fx.state),
                                   torch.randint(0, 256, (4, 32), generator=torch.Generator().manual_seed(
                                       7000 + 10 * ARCHS.index(arch) + 1000)))
    assert set(stats) == set(fx.stats) and all(torch.equal(stats[k], fx.stats[k]) for k in stats)


@pytest.mark.parametrize("not_converted", [[], ["model.layers.1.mlp.down_proj"]], ids=["all", "one_left_out"])
@pytest.mark.parametrize("arch", ARCHS)
def test_written_config_parses_in_transformers(arch, not_converted, tmp_path):
    transformers = pytest.importorskip("transformers")
    from awq_quantizer.main import write_autoawq_configs

    class Loader:
        model_path = mc.fixture(arch).dir

    write_autoawq_configs(str(tmp_path), argparse.Namespace(symmetric=False, group_size=32), Loader(),
                          not_converted)
    cfg = transformers.AutoConfig.from_pretrained(str(tmp_path))
    assert cfg.model_type == arch and cfg.num_hidden_layers == 2
    assert cfg.num_key_value_heads == (2 if arch == "mistral" else 4)
    qc = cfg.quantization_config
    qc = qc if isinstance(qc, dict) else qc.to_dict()
    assert qc["quant_method"] == "awq"
    awq = transformers.AwqConfig(**{k: v for k, v in qc.items() if k != "quant_method"})
    assert (awq.bits, awq.group_size, awq.zero_point) == (4, 32, True)
    assert str(awq.to_dict()["version"]).lower().endswith("gemm")
    assert (awq.modules_to_not_convert or []) == not_converted
    with open(tmp_path / "quant_config.json") as f:
        q = json.load(f)
    assert (q["w_bit"], q["q_group_size"], q["zero_point"], q["version"]) == (4, 32, True, "GEMM")
    assert q.get("modules_to_not_convert", []) == not_converted


def test_reader_inverts_the_packers():
    """The reader against the packers written next to it (both from the layouts' descriptions): a
    round trip, and by hand one word of each layout."""
    g = torch.Generator().manual_seed(5)
    q = torch.randint(0, 16, (16, 64), generator=g)
    z = torch.randint(0, 16, (16, 2), generator=g)
    s = torch.rand(16, 2, generator=g, dtype=torch.float64) + 0.5
    qw, qz = mc.pack_gemm(q, z)
    assert qw.shape == (64, 2) and qz.shape == (2, 2)
    want = (q - z.repeat_interleave(32, 1)).double() * s.repeat_interleave(32, 1)
    assert torch.equal(dequant_gemm(qw, qz, s.t().contiguous(), 32), want)
    # word 0 of input row 0 holds output columns 0, 2, 4, 6, 1, 3, 5, 7 from the low nibble up
    word = sum(int(q[n, 0]) << (4 * i) for i, n in enumerate((0, 2, 4, 6, 1, 3, 5, 7)))
    assert int(qw[0, 0]) & 0xFFFFFFFF == word
    # packed: element k of a row in nibble k % 8 of word k // 8, stored q - qmin
    row = torch.arange(16).reshape(1, 16)
    words = torch.tensor([[0x76543210, 0xFEDCBA98 - (1 << 32)]], dtype=torch.int32)
    r = {"qweight": words, "qzeros": torch.tensor([[3]], dtype=torch.int32),
         "scales": torch.tensor([[0.5]], dtype=torch.float16), "bits": torch.tensor(4),
         "group_size": torch.tensor(16), "symmetric": torch.tensor(False), "shape": torch.tensor([16])}
    assert torch.equal(dequant_packed(r), ((row - 3).double() * 0.5).reshape(16))
    r["symmetric"] = torch.tensor(True)                      # fields hold q + 8 and z + 8
    assert torch.equal(dequant_packed(r), ((row - 3).double() * 0.5).reshape(16))


@pytest.mark.parametrize("group_size", [32, 64])
@pytest.mark.parametrize("arch", ARCHS)
def test_layout_and_zero_point_mutations_exceed_theta(arch, group_size):
    fx = mc.fixture(arch)
    et = mc.e_textbook(arch, "autoawq", group_size)
    gemm = mc.textbook_gemm(fx, group_size)
    rest = {k: v for k, v in fx.source.items() if k not in gemm}
    assert len(gemm) == 14
    es = {k: fx.e(s) for k, s in mc.layout_mutations(fx, gemm, group_size, rest).items()}
    print(f"{arch} gs {group_size}: e_textbook {et:.3e}  " +
          "  ".join(f"{k} {v / et:.2f}" for k, v in es.items()))
    assert abs(es["none"] - et) <= 1e-12                        # pack + read is the identity
    assert 1e-3 < et < 0.05                                      # the quantization is visible and small
    assert 1.0 < mc.THETA <= min(es["identity_nibble_order"], es["zero_point_plus_1"]) / et / mc.THETA
    assert es["identity_nibble_order"] > mc.THETA * et
    assert es["zero_point_plus_1"] > mc.THETA * et


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("arch", ARCHS)
def test_fold_mutations_exceed_the_equivalence_bound(arch, dtype):
    fx = mc.fixture(arch)
    scales, written = mc.host_fold(fx, dtype)
    assert ("model.layers.0.self_attn.v_proj.weight.row_scale" in scales) == (arch != "mistral")
    es = {k: fx.e(s) for k, s in mc.fold_mutations(fx, scales, written).items()}
    print(f"{arch} {dtype}: " + "  ".join(f"{k} {v:.3e}" for k, v in es.items()))
    bound = mc.fold_bound(fx, dtype)
    assert set(es) == {"none", "source_norm_kept", "mlp_out_fold_inverted"} | (
        {"v_bias_fold_dropped"} if arch == "qwen2" else set())
    assert es.pop("none") <= bound
    for label, e in es.items():
        assert e > bound, label
