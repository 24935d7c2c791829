"""The calibration pass on the host (awq_quantizer/calibration, awq_quantizer/calibrate.py, main
--calib_ids): no GPU, no kernel.

The forward driver takes its three memory-bound ops as injected callables; here they are torch
compositions in float64, so the driver itself — block walk, micro-batching, RoPE, GQA, biases, the
shared accumulators and their naming — is judged against the statistics transformers' own classes
recorded in tests/golden/model_*/stats.safetensors (float64 forward hooks, stored as fp32).  The
calibration ids are not stored; make_golden_model.py's recipe regenerates them.

Metric: E = max over the 30 tensors of max|got - ref| / max|ref|.  A float64 forward reproduces
the fixture to its fp32 storage rounding (measured 6.6e-8 / 6.8e-8 / 4.1e-8); asserted E <= 1e-6.
"""
import json
import os
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import load_file, save_file

import model_cases as mc

SEEDS = {"llama": 7000, "mistral": 7010, "qwen2": 7020}


def calib_ids(arch: str) -> torch.Tensor:
    return torch.randint(0, 256, (4, 32), generator=torch.Generator().manual_seed(SEEDS[arch] + 1000))


def metric_e(got, ref_flat) -> float:
    worst = 0.0
    for name, (m, s) in got.items():
        for key, t in ((name + ".x_mean", m), (name + ".x_sq", s)):
            r = ref_flat[key].double()
            worst = max(worst, float((t.double() - r).abs().max() / r.abs().max()))
    return worst


class TorchAcc:
    def __init__(self, K):
        self.a = torch.zeros(K, dtype=torch.float64)
        self.s = torch.zeros(K, dtype=torch.float64)
        self.n = 0

    def add(self, x):
        x = x.double()
        self.a += x.abs().sum(0)
        self.s += (x * x).sum(0)
        self.n += x.shape[0]

    def finish(self):
        return (self.a / self.n).float(), (self.s / self.n).float()


class TorchOps:
    """The three injected ops as torch compositions (any dtype, CPU)."""

    def __init__(self, act=F.silu):
        self.act = act
        self.calls = []

    def new_acc(self, K):
        return TorchAcc(K)

    def rmsnorm(self, x, weight, eps, acc, fused):
        self.calls.append(("rmsnorm", x.shape[0], fused))
        out = weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))
        if acc is not None:
            acc.add(out)
        return out

    def swiglu(self, gate, up, acc, fused):
        out = self.act(gate) * up
        acc.add(out)
        return out

    def accum(self, x, acc):
        acc.add(x)


def run_host(model_dir, ids, dtype=torch.float64, batch_tokens=8192, ops=None):
    from awq_quantizer.calibration import calibrate_model
    return calibrate_model(model_dir, ids, compute_dtype=dtype, batch_tokens=batch_tokens, device="cpu",
                           ops=ops or TorchOps())


def write_model(tmp_path, arch="llama", config_edit=None, drop=()):
    fx = mc.fixture(arch)
    d = tmp_path / f"model_{arch}"
    d.mkdir(exist_ok=True)
    save_file({k: v for k, v in fx.state.items() if k not in drop}, str(d / "model.safetensors"),
              metadata={"format": "pt"})
    cfg = json.loads(json.dumps(fx.config))
    if config_edit:
        config_edit(cfg)
    with open(d / "config.json", "w") as f:
        json.dump(cfg, f)
    return str(d)


# ---------------------------------------------------------------- 1. the driver against transformers' statistics
@pytest.mark.parametrize("arch", mc.ARCHS)
def test_float64_driver_reproduces_recorded_statistics(arch):
    fx = mc.fixture(arch)
    got = run_host(fx.dir, calib_ids(arch))
    assert {n + s for n in got for s in (".x_mean", ".x_sq")} == set(fx.stats)
    assert len(fx.stats) == 30
    for name, (m, s) in got.items():
        assert m.dtype == s.dtype == torch.float32 and m.shape == s.shape == fx.stats[name + ".x_mean"].shape
    e = metric_e(got, fx.stats)
    print(f"{arch}: E = {e:.2e}")
    assert e <= 1e-6
    # q / k / v and gate / up read one input: one accumulator, the same vectors
    p = "model.layers.1."
    for a, b in (("self_attn.q_proj", "self_attn.k_proj"), ("self_attn.q_proj", "self_attn.v_proj"),
                 ("mlp.gate_proj", "mlp.up_proj")):
        assert torch.equal(got[p + a + ".weight"][0], got[p + b + ".weight"][0])


def test_the_metric_sees_a_wrong_activation():
    fx = mc.fixture("llama")
    e = metric_e(run_host(fx.dir, calib_ids("llama"), ops=TorchOps(act=F.gelu)), fx.stats)
    assert e > 0.1          # gelu for silu: 0.23 in fp32


# ---------------------------------------------------------------- 2. micro-batching
@pytest.mark.parametrize("arch", mc.ARCHS)
def test_micro_batching_does_not_change_the_statistics(arch):
    fx = mc.fixture(arch)
    ids = calib_ids(arch)
    a_ops, b_ops = TorchOps(), TorchOps()
    a = run_host(fx.dir, ids, batch_tokens=32, ops=a_ops)
    b = run_host(fx.dir, ids, batch_tokens=128, ops=b_ops)
    assert {c[1] for c in a_ops.calls} == {32} and {c[1] for c in b_ops.calls} == {128}
    assert len(a_ops.calls) == 4 * len(b_ops.calls)
    flat_b = {n + k: t for n, (m, s) in b.items() for k, t in ((".x_mean", m), (".x_sq", s))}
    e = metric_e(a, flat_b)
    print(f"{arch}: E(batch_tokens 32 vs 128) = {e:.2e}")
    assert e <= 1e-12


def test_micro_batch_plan():
    from awq_quantizer.calibration import plan_micro_batches
    assert plan_micro_batches(128, 512, 8192) == ([(i, i + 16) for i in range(0, 128, 16)], True)
    assert plan_micro_batches(4, 32, 64) == ([(0, 2), (2, 4)], False)          # 64 tokens: no whole block
    assert plan_micro_batches(4, 32, 8192) == ([(0, 4)], True)                 # one (last) call
    spans, fused = plan_micro_batches(40, 96, 1000)                            # 8 sequences = 3 blocks
    assert fused and all((b - a) == 8 for a, b in spans)
    assert plan_micro_batches(3, 100, 150) == ([(0, 1), (1, 2), (2, 3)], False)


# ---------------------------------------------------------------- 3. config handling
def _refused(tmp_path, edit, ids=None, arch="llama"):
    from awq_quantizer.calibration import CalibrationConfigError
    d = write_model(tmp_path, arch, edit)
    with pytest.raises(CalibrationConfigError) as ei:
        run_host(d, calib_ids(arch) if ids is None else ids)
    return str(ei.value)


def test_refusals_name_the_key(tmp_path, monkeypatch):
    from awq_quantizer.model_loading import safetensors_loader
    # refused before the model is read: the loader must never be constructed
    monkeypatch.setattr(safetensors_loader.SafetensorsLoader, "__init__",
                        lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model was read")))
    assert "rope_parameters.rope_type" in _refused(
        tmp_path, lambda c: c["rope_parameters"].update(rope_type="yarn", factor=4.0))
    assert "rope_scaling" in _refused(
        tmp_path, lambda c: (c.pop("rope_parameters"), c.update(rope_theta=1e4, rope_scaling={"type": "linear",
                                                                                                "factor": 2.0})))
    assert "model_type" in _refused(tmp_path, lambda c: c.update(model_type="gemma"))
    assert "sliding_window" in _refused(tmp_path, lambda c: c.update(sliding_window=16), arch="mistral")
    assert "vocab_size" in _refused(tmp_path, lambda c: None, ids=torch.full((2, 8), 256, dtype=torch.int64))
    assert "max_position_embeddings" in _refused(tmp_path, lambda c: None, ids=torch.zeros((1, 65), dtype=torch.int64))


def test_config_keys_are_read(tmp_path):
    from awq_quantizer.calibration import parse_config
    fx = mc.fixture("qwen2")
    c = parse_config(fx.config)
    assert (c.eps, c.rope_theta, c.head_dim, c.num_kv_heads) == (1e-6, 1000000.0, 32, 4)
    assert c.sliding_window is None or not fx.config.get("use_sliding_window", False)
    old = {k: v for k, v in fx.config.items() if k != "rope_parameters"}
    old.update(rope_theta=12345.0, rope_scaling=None)
    assert parse_config(old).rope_theta == 12345.0          # top-level rope_theta (transformers 4 configs)
    assert parse_config(mc.fixture("mistral").config).num_kv_heads == 2


def test_tied_embeddings_without_lm_head_give_no_lm_head_keys(tmp_path):
    d = write_model(tmp_path, "llama", lambda c: c.update(tie_word_embeddings=True), drop=("lm_head.weight",))
    ops = TorchOps()
    got = run_host(d, calib_ids("llama"), ops=ops)
    assert "lm_head.weight" not in got and len(got) == 14
    assert len([c for c in ops.calls if c[0] == "rmsnorm"]) == 4        # the final norm never ran
    fx = mc.fixture("llama")
    assert metric_e(got, fx.stats) <= 1e-6


def _golden_rope():
    with open(os.path.join(mc.GOLDEN, "calib", "rope_llama3.json")) as f:
        return json.load(f)["cases"]


def test_llama3_inverse_frequencies_equal_the_recorded_ones():
    from awq_quantizer.calibration import parse_config, rope_inv_freq
    cases = _golden_rope()
    assert [c["config"]["head_dim"] for c in cases] == [64, 128]
    for case in cases:
        cfg = parse_config(case["config"])
        assert cfg.rope_type == "llama3"
        got = rope_inv_freq(cfg)
        want = torch.tensor([struct.unpack(">f", bytes.fromhex(h))[0] for h in case["inv_freq_bits"]])
        assert got.dtype == torch.float32 and torch.equal(got, want)
        plain = rope_inv_freq(parse_config({**case["config"], "rope_parameters": {"rope_theta": 500000.0}}))
        assert torch.equal(plain[:8], got[:8]) and not torch.equal(plain, got)     # high frequencies are kept


def test_llama3_inverse_frequencies_equal_transformers():
    transformers = pytest.importorskip("transformers")
    from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
    from awq_quantizer.calibration import parse_config, rope_inv_freq
    for case in _golden_rope():
        kw = {k: v for k, v in case["config"].items() if k != "model_type"}
        config = transformers.LlamaConfig(intermediate_size=256, **kw)
        want, factor = ROPE_INIT_FUNCTIONS["llama3"](config, "cpu")
        assert factor == 1.0
        assert torch.equal(rope_inv_freq(parse_config(case["config"])), want.float())


# ---------------------------------------------------------------- 4. ids readers and the CLIs
def test_ids_readers(tmp_path):
    from awq_quantizer.calibration import read_input_ids
    ids = calib_ids("llama")
    st, npy = str(tmp_path / "ids.safetensors"), str(tmp_path / "ids.npy")
    save_file({"input_ids": ids}, st)
    np.save(npy, ids.numpy())
    assert torch.equal(read_input_ids(st), ids) and torch.equal(read_input_ids(npy), ids)
    bad = {"rank": ids[0], "dtype": ids.to(torch.int32), "empty": ids[:0]}
    for label, t in bad.items():
        p = str(tmp_path / f"{label}.safetensors")
        save_file({"input_ids": t.contiguous()}, p)
        with pytest.raises(ValueError, match="input_ids"):
            read_input_ids(p)
        q = str(tmp_path / f"{label}.npy")
        np.save(q, t.numpy())
        with pytest.raises(ValueError, match="input_ids"):
            read_input_ids(q)
    save_file({"ids": ids}, str(tmp_path / "noname.safetensors"))
    with pytest.raises(ValueError, match="input_ids"):
        read_input_ids(str(tmp_path / "noname.safetensors"))


def _word_tokenizer(path, words):
    tokenizers = pytest.importorskip("tokenizers")
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace
    vocab = {w: i for i, w in enumerate(["[UNK]"] + words)}
    tok = tokenizers.Tokenizer(WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = Whitespace()
    tok.save(path)
    return vocab


def test_text_file_chunking(tmp_path):
    from awq_quantizer import calibrate
    words = [f"w{i}" for i in range(50)]
    d = tmp_path / "m"
    d.mkdir()
    vocab = _word_tokenizer(str(d / "tokenizer.json"), words)
    text = " ".join(words[i % 50] for i in range(103)) + "\n"
    (tmp_path / "t.txt").write_text(text)
    base = ["--model_id", str(d), "--output", "o", "--text_file", str(tmp_path / "t.txt")]
    args = calibrate.build_parser().parse_args(base + ["--seq_len", "10", "--n_samples", "4"])
    ids = calibrate.load_ids(args)
    want = torch.tensor([vocab[words[i % 50]] for i in range(40)]).view(4, 10)
    assert ids.dtype == torch.int64 and torch.equal(ids, want)
    args = calibrate.build_parser().parse_args(base + ["--seq_len", "10", "--n_samples", "128"])
    assert calibrate.load_ids(args).shape == (10, 10)            # 103 tokens: ten whole blocks, the tail dropped
    args = calibrate.build_parser().parse_args(base + ["--seq_len", "512"])
    with pytest.raises(ValueError, match="seq_len"):
        calibrate.load_ids(args)


def test_cli_argument_errors_exit_1_before_device_work(tmp_path, monkeypatch, caplog):
    from awq_quantizer import calibrate, calibration
    monkeypatch.setattr(calibration, "calibrate_model",
                        lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work started")))
    d = write_model(tmp_path, "llama")
    ids_path = str(tmp_path / "ids.safetensors")
    save_file({"input_ids": calib_ids("llama")}, ids_path)
    out = str(tmp_path / "stats.safetensors")
    ok = ["--model_id", d, "--output", out]
    (tmp_path / "t.txt").write_text("a b c")
    big = str(tmp_path / "big.safetensors")
    save_file({"input_ids": torch.full((1, 8), 999, dtype=torch.int64)}, big)
    wrong = str(tmp_path / "wrong.safetensors")
    save_file({"input_ids": torch.zeros(8, dtype=torch.int64)}, wrong)
    cases = {
        "no source": ok,
        "two sources": ok + ["--input_ids", ids_path, "--text_file", str(tmp_path / "t.txt")],
        "missing ids file": ok + ["--input_ids", str(tmp_path / "nope.safetensors")],
        "wrong rank": ok + ["--input_ids", wrong],
        "ids beyond the vocabulary": ok + ["--input_ids", big],
        "no tokenizer.json": ok + ["--text_file", str(tmp_path / "t.txt")],
        "bad batch_tokens": ok + ["--input_ids", ids_path, "--batch_tokens", "0"],
        "bad dtype": ok + ["--input_ids", ids_path, "--compute_dtype", "int8"],
        "no model dir": ["--model_id", str(tmp_path / "none"), "--output", out, "--input_ids", ids_path],
    }
    for label, argv in cases.items():
        assert calibrate.main(argv) == 1, label
    assert not os.path.exists(out)


def test_cli_on_the_cpu_fails_loudly(tmp_path):
    from awq_quantizer import calibrate
    d = write_model(tmp_path, "llama")
    ids_path = str(tmp_path / "ids.safetensors")
    save_file({"input_ids": calib_ids("llama")}, ids_path)
    out = str(tmp_path / "stats.safetensors")
    assert calibrate.main(["--model_id", d, "--output", out, "--input_ids", ids_path, "--device", "cpu"]) == 1   # no CPU fallback
    assert not os.path.exists(out)


def test_calib_ids_with_act_stats_is_refused(tmp_path, monkeypatch):
    from awq_quantizer import main as M
    monkeypatch.setattr(M, "load_model_from_hub",
                        lambda *a, **k: (_ for _ in ()).throw(AssertionError("the model was opened")))
    fx = mc.fixture("llama")
    ids_path = str(tmp_path / "ids.safetensors")
    save_file({"input_ids": calib_ids("llama")}, ids_path)
    rc = M.main(["--model_id", fx.dir, "--output_dir", str(tmp_path / "out"), "--scale_method", "awq", "--device", "cpu",
                 "--act_stats", fx.stats_path, "--calib_ids", ids_path, "--log_level", "CRITICAL"])
    assert rc == 1


def test_save_act_stats_round_trips_through_load_act_stats(tmp_path):
    from awq_quantizer.calibration import save_act_stats
    from awq_quantizer.main import load_act_stats
    fx = mc.fixture("llama")
    got = run_host(fx.dir, calib_ids("llama"))
    path = str(tmp_path / "stats.safetensors")
    save_act_stats(got, path)
    back = load_act_stats(path)
    assert set(back) == set(got)
    assert all(torch.equal(back[n][0], got[n][0]) and torch.equal(back[n][1], got[n][1]) for n in got)
    assert set(load_file(path)) == set(fx.stats)
