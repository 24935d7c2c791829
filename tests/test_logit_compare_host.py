"""CPU-only tests of the evaluation feature's host layer (include/awq_hip.h awq_logit_compare,
awq_quantizer/evaluation, python -m awq_quantizer.evaluate): the symbol is exported
by both libraries and bound, every refusal comes before a launch, the CLI's flag rules, the target
shift, the aggregates, the driver with float64 torch ops against the fixtures' recorded float64
logits (tied head included), and the written-directory loader in the three formats."""
import ctypes
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import save_file

import checkpoint_reader as cr
import model_cases as mc
from model_forward import model_forward

BF16, F16, F32, F64, I32 = 0, 1, 2, 3, 4   # include/awq_hip.h AWQ_DTYPE_*
OK, EINVAL, EUNSUPPORTED = 0, 1, 2


def _call(lib, *, ref=0x1000, q=0, dtype=BF16, T=4, V=16, sr=None, sq=None):
    P = ctypes.c_void_p
    return lib.awq_logit_compare(P(ref), P(q), dtype, T, V, V if sr is None else sr, V if sq is None else sq,
                                 P(0), P(0), P(0), P(0), P(0), P(0), None)


def test_symbol_exported_by_both_libraries_and_bound():
    from awq_quantizer import _hip
    assert len(_hip.SIGNATURES["awq_logit_compare"][1]) == 14
    for lib in (_hip.load_library(), _hip.load_diag_library()):
        assert hasattr(lib, "awq_logit_compare")
        assert lib.awq_abi_version() == 17          # additive symbol: the ABI number stays
    assert callable(_hip.logit_compare)


REFUSALS = [
    (dict(dtype=F64), EUNSUPPORTED), (dict(dtype=I32), EUNSUPPORTED), (dict(dtype=-1), EUNSUPPORTED),
    (dict(T=-1), EINVAL), (dict(V=0), EINVAL), (dict(V=-3), EINVAL),
    (dict(sr=15), EINVAL), (dict(q=0x2000, sq=15), EINVAL), (dict(sr=0), EINVAL),
    (dict(T=1 << 40, sr=1 << 21, V=16), EINVAL), (dict(q=0x2000, T=1 << 40, sq=1 << 21), EINVAL),
    (dict(V=1 << 31, sr=1 << 31), EINVAL), (dict(V=(1 << 31) + 5, sr=1 << 32), EINVAL),
    (dict(ref=0), EINVAL),
]


def test_refusals_come_before_any_launch():
    """No device here: a call that got as far as a launch would not return these codes."""
    from awq_quantizer import _hip
    lib = _hip.load_library()
    for kw, code in REFUSALS:
        assert _call(lib, **kw) == code, kw
        assert _hip.last_error() != "", kw
    assert "stride" in (_call(lib, sr=15), _hip.last_error())[1]
    assert "2^60" in (_call(lib, T=1 << 40, sr=1 << 21), _hip.last_error())[1]


def test_empty_returns_before_the_pointers():
    from awq_quantizer import _hip
    lib = _hip.load_library()
    assert _call(lib, T=0, ref=0) == OK and _hip.last_error() == ""
    assert _call(lib, T=0, ref=0, sr=3, V=16) == OK         # T == 0 is answered before the strides are judged
    assert _call(lib, T=0, dtype=F64) == EUNSUPPORTED       # but after the dtype and the shape's signs
    assert _call(lib, T=0, V=0) == EINVAL


def test_q_stride_is_ignored_without_q():
    """The single-model form: q_row_stride < V is no refusal (the NULL ref is what is refused)."""
    from awq_quantizer import _hip
    lib = _hip.load_library()
    assert _call(lib, ref=0, q=0, sq=0) == EINVAL and "ref" in _hip.last_error()


# ------------------------------------------------------------------ targets and aggregates
def test_targets_shift_within_each_sequence():
    from awq_quantizer.evaluation import shifted_targets
    ids = torch.tensor([[5, 6, 7], [8, 9, 10]])
    assert shifted_targets(ids).tolist() == [6, 7, -1, 9, 10, -1]
    assert shifted_targets(torch.tensor([[3]])).tolist() == [-1]


def test_aggregates_from_known_vectors():
    from awq_quantizer.evaluation import aggregate
    targets = torch.tensor([2, 0, -1, 1])
    per = {"nll_ref": torch.tensor([1.0, 2.0, 0.0, 3.0]), "nll_q": torch.tensor([2.0, 2.0, 0.0, 5.0]),
           "kl": torch.tensor([0.5, 0.0, 0.25, 0.25]), "argmax_ref": torch.tensor([2, 1, 3, 1], dtype=torch.int32),
           "argmax_q": torch.tensor([2, 0, 3, 0], dtype=torch.int32)}
    r = aggregate(per, targets)
    assert (r["n_positions"], r["n_tokens_scored"], r["nonfinite_rows"]) == (4, 3, 0)
    assert r["nll_ref_sum"] == 6.0 and r["nll_q_sum"] == 9.0
    assert r["ppl_ref"] == math.exp(2.0) and r["ppl_q"] == math.exp(3.0) and r["ppl_ratio"] == math.exp(3.0) / math.exp(2.0)
    assert r["kl_mean"] == 0.25 and r["kl_max"] == 0.5
    assert r["top1_agreement"] == 0.5                      # every position counts
    assert r["top1_accuracy_ref"] == 2 / 3 and r["top1_accuracy_q"] == 2 / 3
    single = aggregate({k: per[k] for k in ("nll_ref", "argmax_ref")}, targets)
    assert "ppl_q" not in single and single["ppl_ref"] == math.exp(2.0)
    per["argmax_q"][1] = -1
    assert aggregate(per, targets)["nonfinite_rows"] == 1


def test_aggregates_with_nothing_scored():
    from awq_quantizer.evaluation import aggregate
    per = {"nll_ref": torch.zeros(2), "nll_q": torch.zeros(2), "kl": torch.tensor([0.5, 1.5]),
           "argmax_ref": torch.tensor([0, 1], dtype=torch.int32), "argmax_q": torch.tensor([0, 0], dtype=torch.int32)}
    r = aggregate(per, torch.tensor([-1, -1]))
    assert r["n_tokens_scored"] == 0 and r["n_positions"] == 2 and r["nll_ref_sum"] == 0.0
    assert all(math.isnan(r[k]) for k in ("ppl_ref", "ppl_q", "ppl_ratio", "top1_accuracy_ref", "top1_accuracy_q"))
    assert r["kl_mean"] == 1.0 and r["top1_agreement"] == 0.5


# ------------------------------------------------------------------ the CLI's flag rules
@pytest.fixture(scope="module")
def llama_dir(tmp_path_factory):
    return _model_dir(tmp_path_factory.mktemp("llama_src"), mc.fixture("llama"))


def _model_dir(d, fx, state=None, config=None):
    save_file({k: v.contiguous() for k, v in (state or fx.state).items()}, str(d / "model.safetensors"),
              metadata={"format": "pt"})
    with open(d / "config.json", "w") as f:
        json.dump(config or fx.config, f)
    save_file({"input_ids": fx.input_ids}, str(d) + "_ids.safetensors")       # beside, not inside, the model
    return str(d)


def test_cli_flag_rules(llama_dir, tmp_path, capsys):
    from awq_quantizer import evaluate
    ids = llama_dir + "_ids.safetensors"
    fx = mc.fixture("llama")
    big = tmp_path / "big.safetensors"
    save_file({"input_ids": torch.full((1, 4), fx.config["vocab_size"], dtype=torch.int64)}, str(big))
    long_ids = tmp_path / "long.safetensors"
    save_file({"input_ids": torch.zeros((1, fx.config["max_position_embeddings"] + 1), dtype=torch.int64)}, str(long_ids))
    other = tmp_path / "other"
    other.mkdir()
    for label, cfg in (("gpt2", dict(fx.config, model_type="gpt2")),
                       ("yarn", dict(fx.config, rope_scaling={"rope_type": "yarn", "factor": 2.0},
                                     rope_parameters=dict(fx.config.get("rope_parameters") or {}, rope_type="yarn"))),
                       ("window", dict(fx.config, model_type="mistral", sliding_window=2))):
        (other / label).mkdir()
        with open(other / label / "config.json", "w") as f:
            json.dump(cfg, f)
    base = ["--model_id", llama_dir, "--log_level", "CRITICAL"]
    calls = []

    def fake(model_dir, ids, **kw):
        calls.append(kw)
        return {"n_positions": 48, "n_tokens_scored": 46, "nonfinite_rows": fake.bad, "ppl_ref": 10.0, "ppl_q": 11.0,
                "ppl_ratio": 1.1, "kl_mean": 0.02, "kl_max": 0.3, "top1_agreement": 0.9}
    fake.bad = 0

    table = [
        (base, 1, "one of the arguments"),                                           # no token source
        (base + ["--input_ids", ids, "--text_file", ids], 1, "not allowed with"),
        (base + ["--input_ids", ids, "--batch_tokens", "0"], 1, None),
        (base + ["--input_ids", ids, "--max_kl", "0.1"], 1, None),                   # a gate without --quantized_dir
        (base + ["--input_ids", ids, "--max_ppl_ratio", "1.5"], 1, None),
        (base + ["--input_ids", ids, "--quantized_dir", str(tmp_path / "missing")], 1, None),
        (base + ["--input_ids", str(tmp_path / "missing.safetensors")], 1, None),
        (base + ["--input_ids", str(big)], 1, None),                                 # ids >= vocab
        (base + ["--input_ids", str(long_ids)], 1, None),                            # above max_position_embeddings
        (["--model_id", str(other / "gpt2"), "--log_level", "CRITICAL", "--input_ids", ids], 1, None),
        (["--model_id", str(other / "yarn"), "--log_level", "CRITICAL", "--input_ids", ids], 1, None),
        (["--model_id", str(other / "window"), "--log_level", "CRITICAL", "--input_ids", ids], 1, None),
        (base + ["--input_ids", ids, "--compute_dtype", "float64"], 1, "invalid choice"),
    ]
    for argv, code, text in table:
        assert evaluate.main(argv, evaluate_fn=fake) == code, argv
        if text:
            assert text in capsys.readouterr().err, argv
    assert calls == []                         # every refusal above came before the model was read
    q = str(other)                             # any existing directory: the fake never opens it
    report = tmp_path / "r" / "eval.json"
    ok = base + ["--input_ids", ids, "--quantized_dir", q]
    assert evaluate.main(ok + ["--report", str(report)], evaluate_fn=fake) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["ppl_ratio"] == 1.1 and calls[-1]["quantized_dir"] == q and calls[-1]["batch_tokens"] == 8192
    saved = json.loads(report.read_text())
    assert saved["result"] == line and saved["args"]["model_id"] == llama_dir and saved["failed"] == []
    assert evaluate.main(ok + ["--max_ppl_ratio", "1.05"], evaluate_fn=fake) == 1
    assert evaluate.main(ok + ["--max_ppl_ratio", "1.1", "--max_kl", "0.02"], evaluate_fn=fake) == 0
    assert evaluate.main(ok + ["--max_kl", "0.01"], evaluate_fn=fake) == 1
    fake.bad = 2
    assert evaluate.main(ok, evaluate_fn=fake) == 1


def test_refused_model_type_reads_no_tensor(tmp_path):
    """The directory holds config.json alone: reading a tensor would fail differently."""
    from awq_quantizer import evaluate
    fx = mc.fixture("llama")
    with open(tmp_path / "config.json", "w") as f:
        json.dump(dict(fx.config, model_type="gpt_neox"), f)
    save_file({"input_ids": fx.input_ids}, str(tmp_path / "ids.safetensors"))
    assert evaluate.main(["--model_id", str(tmp_path), "--input_ids", str(tmp_path / "ids.safetensors"),
                          "--log_level", "CRITICAL"]) == 1


# ------------------------------------------------------------------ the driver with float64 torch ops
class TorchEvalOps:
    """The injected ops as float64 torch compositions (CPU)."""

    def new_acc(self, K):
        raise AssertionError("the evaluation pass takes no statistics")

    def rmsnorm(self, x, weight, eps, acc, fused):
        assert acc is None
        return weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))

    def swiglu(self, gate, up, acc, fused):
        assert acc is None
        return F.silu(gate) * up

    def accum(self, x, acc):
        assert acc is None

    def logit_compare(self, ref, q, targets):
        return restate(ref, q, targets)


def restate(ref, q, targets):
    """include/awq_hip.h awq_logit_compare in float64 torch (finite rows)."""
    lr = torch.log_softmax(ref.double(), -1)
    safe = targets.clamp_min(0)[:, None]
    out = {"nll_ref": torch.where(targets >= 0, -lr.gather(1, safe)[:, 0], torch.zeros(())),
           "argmax_ref": ref.argmax(-1).to(torch.int32), "nll_q": None, "kl": None, "argmax_q": None}
    if q is not None:
        lq = torch.log_softmax(q.double(), -1)
        out.update(nll_q=torch.where(targets >= 0, -lq.gather(1, safe)[:, 0], torch.zeros(())),
                   kl=(lr.exp() * (lr - lq)).sum(-1), argmax_q=q.argmax(-1).to(torch.int32))
    return out


def nll_of_logits(logits, ids):
    """float64 logits [n, seq, V] -> per-token nll [n * seq] with the last position of a sequence +0."""
    from awq_quantizer.evaluation import shifted_targets
    t = shifted_targets(ids)
    return restate(logits.reshape(-1, logits.shape[-1]), None, t)["nll_ref"], t


@pytest.mark.parametrize("arch", mc.ARCHS)
def test_driver_matches_the_recorded_logits(arch, tmp_path):
    from awq_quantizer.evaluation import evaluate_model
    fx = mc.fixture(arch)
    d = _model_dir(tmp_path, fx)
    per = {}
    r = evaluate_model(d, fx.input_ids, compute_dtype="float64", device="cpu", ops=TorchEvalOps(), per_token=per,
                       batch_tokens=16)                       # 48 positions: three head chunks
    want, t = nll_of_logits(fx.logits, fx.input_ids)
    bound = 1e-9 * float(fx.logits.abs().max())
    assert float((per["nll_ref"] - want).abs().max()) <= bound
    assert torch.equal(per["targets"], t) and r["n_positions"] == fx.input_ids.numel()
    assert r["n_tokens_scored"] == fx.input_ids.numel() - fx.input_ids.shape[0]
    assert abs(r["ppl_ref"] - math.exp(float(want.sum()) / r["n_tokens_scored"])) <= 1e-9 * r["ppl_ref"]
    assert "ppl_q" not in r and r["nonfinite_rows"] == 0


def test_driver_with_a_tied_head(tmp_path):
    from awq_quantizer.evaluation import evaluate_model
    fx = mc.fixture("llama")
    state = {k: v for k, v in fx.state.items() if k != "lm_head.weight"}
    assert len(state) == len(fx.state) - 1
    d = _model_dir(tmp_path, fx, state=state, config=dict(fx.config, tie_word_embeddings=True))
    per = {}
    evaluate_model(d, fx.input_ids, compute_dtype="float64", device="cpu", ops=TorchEvalOps(), per_token=per)
    tied = {k: v.double() for k, v in state.items()}
    tied["lm_head.weight"] = tied["model.embed_tokens.weight"]
    logits = model_forward(tied, fx.config, fx.input_ids)
    want, _ = nll_of_logits(logits, fx.input_ids)
    assert float((per["nll_ref"] - want).abs().max()) <= 1e-9 * float(logits.abs().max())
    untied, _ = nll_of_logits(fx.logits, fx.input_ids)
    assert float((per["nll_ref"] - untied).abs().max()) > 1e-3          # the branch is visible


# ------------------------------------------------------------------ the written-directory loader
class ReaderDequant:
    """The loader's `dequant` from tests/checkpoint_reader.py's float64 integer arithmetic."""

    def packed(self, res):
        return cr.dequant_packed(res)

    def reference(self, res):
        rows = res["tensor_q"].shape[0] if res["tensor_q"].dim() > 1 else 1
        g = torch.arange(res["tensor_q"].numel() // rows) // int(res["group_size"])
        tq = res["tensor_q"].reshape(rows, -1).double()
        return ((tq - res["zero_points"].double()[:, g]) * res["scales"].double()[:, g]).reshape(res["tensor_q"].shape)

    def autoawq(self, gemm, group_size, symmetric):
        assert not symmetric
        return cr.dequant_gemm(gemm["qweight"], gemm["qzeros"], gemm["scales"], group_size)

    def unscale(self, w, s):
        return w / s.double()[None, :]


def _pack_rows(v, bits=4):
    per = 32 // bits
    pad = (-v.shape[1]) % per
    v = torch.cat([v.to(torch.int64), torch.zeros(v.shape[0], pad, dtype=torch.int64)], 1).reshape(v.shape[0], -1, per)
    word = (v << torch.arange(0, 32, bits, dtype=torch.int64)).sum(-1)
    return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)


def _stub_results(fx, names, gs, packed, scaled=()):
    """Textbook RTN results in main's dict layout; `scaled` names quantize W * diag(s) and carry input_scale."""
    out = {}
    for n in names:
        w = fx.source[n]
        extra = {}
        if n in scaled:
            s = (torch.arange(w.shape[1], dtype=torch.float32) % 7 + 1) / 4
            w, extra = w * s.double()[None, :], {"input_scale": s}
        q, z, sc = mc.textbook_rtn(w, gs)
        meta = {"bits": torch.tensor(4, dtype=torch.int32), "group_size": torch.tensor(gs, dtype=torch.int32),
                "symmetric": torch.tensor(False)}
        if packed:
            out[n] = {"qweight": _pack_rows(q), "qzeros": _pack_rows(z), "scales": sc.half(),
                      "shape": torch.tensor(list(fx.source[n].shape), dtype=torch.int64), **meta, **extra}
        else:
            out[n] = {"tensor_q": q.to(torch.int32), "zero_points": z.to(torch.int32), "scales": sc.half(), **meta, **extra}
    return out


def _write_chunks(d, results, st):
    names = sorted(results)
    chunks = [names[: len(names) // 2], names[len(names) // 2:]]
    for c, part in enumerate(chunks):
        if st:
            save_file({f"{n}.{k}": v.contiguous() for n in part for k, v in results[n].items()},
                      str(d / f"model_chunk_{c:04d}.safetensors"))
        else:
            torch.save({n: results[n] for n in part}, str(d / f"model_chunk_{c:04d}.pt"))
    with open(d / "metadata.json", "w") as f:
        json.dump({"num_chunks": 2, "format": "safetensors" if st else "pt",
                   "tensor_to_chunk": {n: c for c, part in enumerate(chunks) for n in part}}, f)


def _open(src_dir, qdir):
    from awq_quantizer.evaluation import QuantizedCheckpoint
    from awq_quantizer.model_loading.safetensors_loader import SafetensorsLoader
    loader = SafetensorsLoader(src_dir, logger_level="ERROR")
    return loader, QuantizedCheckpoint(loader, str(qdir), ReaderDequant())


@pytest.mark.parametrize("fmt", ["packed", "reference"])
def test_loader_reads_chunk_directories(fmt, llama_dir, tmp_path):
    fx = mc.fixture("llama")
    names = [n for n in fx.quantized_names("autoawq")]
    scaled = set(names[:2])
    results = _stub_results(fx, names, 32, fmt == "packed", scaled)
    _write_chunks(tmp_path, results, st=fmt == "packed")
    loader, q = _open(llama_dir, tmp_path)
    assert sorted(q.quantized_names()) == sorted(names)
    if fmt == "packed":
        want, _ = cr.read_checkpoint(str(tmp_path))
    else:
        want = {n: ReaderDequant().reference(r) for n, r in results.items()}
    for info in q.tensor_index():
        got = q.read(info)
        assert tuple(got.shape) == tuple(info.shape), info.name
        if info.name in scaled:            # back in the source's domain: the division is the only rounding
            assert torch.equal(got, want[info.name] / results[info.name]["input_scale"].double()[None, :])
            assert not torch.equal(got, want[info.name])
        elif info.name in results:         # integer and fp16 arithmetic: exact
            assert torch.equal(got, want[info.name]), info.name
        else:                              # not in the directory: the source's bytes
            assert torch.equal(got, fx.state[info.name]), info.name
    q.close()
    loader.close()


def test_loader_reads_an_autoawq_directory(llama_dir, tmp_path):
    fx = mc.fixture("llama")
    gemm = mc.textbook_gemm(fx, 32)
    flat = {}
    for n, r in gemm.items():
        for k, v in r.items():
            flat[f"{n[: -len('.weight')]}.{k}"] = v.half() if k == "scales" else v
    norm = "model.layers.0.input_layernorm.weight"
    flat[norm] = (fx.state[norm].float() * 0.5).to(fx.state[norm].dtype)        # a folded norm: read as written
    save_file({k: v.contiguous() for k, v in flat.items()}, str(tmp_path / "model.safetensors"))
    with open(tmp_path / "quant_config.json", "w") as f:
        json.dump({"w_bit": 4, "q_group_size": 32, "zero_point": True, "version": "gemm"}, f)
    loader, q = _open(llama_dir, tmp_path)
    want, _ = cr.read_checkpoint(str(tmp_path))
    assert sorted(q.quantized_names()) == sorted(gemm)
    for info in q.tensor_index():
        got = q.read(info)
        if info.name in gemm:
            assert torch.equal(got, want[info.name]), info.name
        elif info.name == norm:
            assert torch.equal(got, flat[norm])
        else:
            assert torch.equal(got, fx.state[info.name]), info.name
    q.close()
    loader.close()


def test_driver_on_a_written_directory(llama_dir, tmp_path):
    """Both models through the driver: the float64 metrics of checkpoint_reader + model_forward."""
    from awq_quantizer.evaluation import evaluate_model, shifted_targets
    fx = mc.fixture("llama")
    results = _stub_results(fx, fx.quantized_names("autoawq"), 32, True)
    _write_chunks(tmp_path, results, st=True)
    per = {}
    r = evaluate_model(llama_dir, fx.input_ids, quantized_dir=str(tmp_path), compute_dtype="float64", device="cpu",
                       ops=TorchEvalOps(), dequant=ReaderDequant(), per_token=per)
    state, _ = cr.read_checkpoint(str(tmp_path))
    lq = model_forward({**fx.source, **state}, fx.config, fx.input_ids)
    V = lq.shape[-1]
    want = restate(fx.logits.reshape(-1, V), lq.reshape(-1, V), shifted_targets(fx.input_ids))
    tol = 1e-9 * float(fx.logits.abs().max())
    for k in ("nll_ref", "nll_q", "kl"):
        assert float((per[k] - want[k]).abs().max()) <= tol, k
    assert torch.equal(per["argmax_q"], want["argmax_q"])
    assert r["ppl_ratio"] > 1.0 and r["kl_mean"] > 0 and 0 < r["top1_agreement"] <= 1
    same = evaluate_model(llama_dir, fx.input_ids, quantized_dir=_empty_chunks(tmp_path / "same"),
                          compute_dtype="float64", device="cpu", ops=TorchEvalOps(), dequant=ReaderDequant())
    assert same["kl_mean"] == 0 and same["ppl_ratio"] == 1 and same["top1_agreement"] == 1.0


def _empty_chunks(d):
    """A directory that holds nothing: every tensor comes from the source."""
    d.mkdir()
    with open(d / "metadata.json", "w") as f:
        json.dump({"num_chunks": 0, "format": "safetensors", "tensor_to_chunk": {}}, f)
    return str(d)
