"""CPU-only tests of the quantization-error report's host layer: the two C-ABI symbols are
exported and bound, awq_quant_error validates its arguments before anything launches,
quantization_error keeps dequantize()'s IndexError for small-tensor results, and
awq_quantizer.verify parses its arguments and writes its JSON report (error function stubbed)."""
import ctypes
import json
import math

import pytest
import torch

BF16, F16, F32, F64, I32 = 0, 1, 2, 3, 4   # include/awq_hip.h AWQ_DTYPE_*
EINVAL, EUNSUPPORTED = 1, 2


def _lib():
    from awq_quantizer import _hip
    return _hip.load_library()


def _call(lib, *, w=0x1000, dtype=BF16, rows=4, K=256, gs=128, bits=4, sym=0, qweight=0x2000, qzeros=0x3000,
          scales=0x4000, stats=0x5000, bad=0x6000, work=0x7000, totals=0x8000):
    """awq_quant_error with dummy (never dereferenced: validation fails first) device pointers."""
    P = ctypes.c_void_p
    return lib.awq_quant_error(P(w), dtype, rows, K, gs, bits, sym, P(qweight), P(qzeros), P(scales), P(stats),
                               P(bad), P(work), P(totals), None)


def test_symbols_exported_and_bound():
    from awq_quantizer import _hip
    lib = _lib()
    for name in ("awq_quant_error", "awq_quant_error_work_bytes"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert lib.awq_quant_error_work_bytes.restype is ctypes.c_int64
    assert len(_hip.SIGNATURES["awq_quant_error"][1]) == 15
    assert lib.awq_abi_version() == 17          # additive symbols: the ABI number stays
    assert callable(_hip.quant_error)


def test_work_bytes():
    lib = _lib()
    assert lib.awq_quant_error_work_bytes(4096, 4096, 128) == 8 * 5 * 128      # 131072 groups = 128 blocks
    assert lib.awq_quant_error_work_bytes(3, 256, 128) == 40
    assert lib.awq_quant_error_work_bytes(4, 250, 100) > 0                     # tail group
    assert lib.awq_quant_error_work_bytes(2, 1024, 512) > 0
    assert lib.awq_quant_error_work_bytes(2, 1024, 513) < 0
    assert lib.awq_quant_error_work_bytes(2, 1024, 0) < 0
    assert lib.awq_quant_error_work_bytes(-1, 1024, 128) < 0
    assert lib.awq_quant_error_work_bytes(1 << 31, 128, 128) < 0               # rows * G past int32


@pytest.mark.parametrize("kw,code", [
    (dict(w=0), EINVAL), (dict(qweight=0), EINVAL), (dict(qzeros=0), EINVAL), (dict(scales=0), EINVAL),
    (dict(stats=0), EINVAL), (dict(bad=0), EINVAL), (dict(work=0), EINVAL),
    (dict(bits=3), EINVAL), (dict(bits=16), EINVAL),
    (dict(gs=0), EINVAL), (dict(gs=-128), EINVAL), (dict(gs=513), EUNSUPPORTED),
    (dict(dtype=F64), EUNSUPPORTED), (dict(dtype=I32), EINVAL), (dict(dtype=8), EINVAL), (dict(dtype=-1), EINVAL),
    (dict(rows=-1), EINVAL), (dict(K=-256), EINVAL),
    (dict(w=0x1001), EINVAL), (dict(scales=0x4001), EINVAL), (dict(totals=0x8004), EINVAL),
])
def test_invalid_arguments_are_reported_before_any_launch(kw, code):
    from awq_quantizer import _hip
    lib = _lib()
    assert _call(lib, **kw) == code
    assert _hip.last_error() != ""


def _quantizer():
    from awq_quantizer.quantization import AWQQuantizer
    return AWQQuantizer(bits=4, group_size=128, symmetric=False, device="cpu", logger_level="ERROR")


def test_quantization_error_small_tensor_result_raises_index_error():
    """0-d / 1-d scales (awq.py:130-171 results) are no group results: IndexError, as dequantize()."""
    q = _quantizer()
    x = torch.randn(16)
    res = {"tensor_q": torch.zeros(16, dtype=torch.int32), "scales": torch.tensor(0.1, dtype=torch.float16),
           "zero_points": torch.tensor(0, dtype=torch.int32), "bits": torch.tensor(4, dtype=torch.int32),
           "group_size": torch.tensor(128, dtype=torch.int32), "symmetric": torch.tensor(False)}
    with pytest.raises(IndexError):
        q.quantization_error(x, res)
    res["scales"] = torch.full((4,), 0.1, dtype=torch.float16)
    res["zero_points"] = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(IndexError):
        q.quantization_error(x.reshape(4, 4), res)
    with pytest.raises(ValueError):
        q.quantization_error(torch.zeros(16, dtype=torch.int32), res)


def test_error_report_numbers():
    from awq_quantizer.quantization.awq import error_report
    r = error_report(100, [5.0, 0.5, 50.0, 0.25, 10.0])
    assert (r["numel"], r["nonfinite"]) == (100, 10) and isinstance(r["nonfinite"], int)
    assert r["mean_abs_error"] == 5.0 / 90 and r["mse"] == 0.5 / 90 and r["max_abs_error"] == 0.25
    assert r["snr_db"] == 10.0 * math.log10(100.0)
    z = error_report(8, [0.0, 0.0, 3.0, 0.0, 0.0])
    assert z["snr_db"] == math.inf and z["mean_abs_error"] == 0.0
    n = error_report(8, [0.0, 0.0, 0.0, 0.0, 8.0])
    assert math.isnan(n["mean_abs_error"]) and math.isnan(n["mse"]) and n["snr_db"] == math.inf


def test_verify_argument_parsing():
    from awq_quantizer import verify
    a = verify.parse_args(["--model_id", "src", "--quantized_dir", "out"])
    assert (a.model_id, a.quantized_dir, a.report, a.device, a.worst) == ("src", "out", None, "cuda:0", 5)
    a = verify.parse_args(["--model_id", "s", "--quantized_dir", "o", "--report", "r.json", "--device", "cuda:1",
                           "--worst", "2"])
    assert (a.report, a.device, a.worst) == ("r.json", "cuda:1", 2)
    with pytest.raises(SystemExit):
        verify.parse_args(["--model_id", "src"])


def _write_model(tmp_path):
    from safetensors.torch import save_file
    g = torch.Generator().manual_seed(5)
    tensors = {"a.weight": torch.randn(4, 256, generator=g).to(torch.bfloat16),
               "b.weight": torch.randn(2, 128, generator=g).to(torch.float16)}
    src = tmp_path / "src"
    src.mkdir()
    save_file(tensors, str(src / "model.safetensors"))
    return str(src), tensors


def _fake_results(tensors, packed):
    out = {}
    for name, t in tensors.items():
        rows, K = t.shape
        common = {"scales": torch.ones((rows, K // 128), dtype=torch.float16), "bits": torch.tensor(4, dtype=torch.int32),
                  "group_size": torch.tensor(128, dtype=torch.int32), "symmetric": torch.tensor(False)}
        if packed:
            out[name] = dict(common, qweight=torch.zeros((rows, K // 8), dtype=torch.int32),
                             qzeros=torch.zeros((rows, 1), dtype=torch.int32),
                             shape=torch.tensor([rows, K], dtype=torch.int64))
        else:
            out[name] = dict(common, tensor_q=torch.zeros((rows, K), dtype=torch.int32),
                             zero_points=torch.zeros((rows, K // 128), dtype=torch.int32))
    return out


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("st", [False, True])
def test_verify_writes_json_report_with_stubbed_error_function(tmp_path, packed, st):
    from awq_quantizer import verify
    from awq_quantizer.main import save_model_in_chunks
    from awq_quantizer.quantization.awq import error_report
    src, tensors = _write_model(tmp_path)
    out = tmp_path / "out"
    save_model_in_chunks(_fake_results(tensors, packed), str(out), chunk_size=1, use_safetensors=st)
    seen = {}

    def stub(tensor, result):
        seen[tuple(tensor.shape)] = sorted(result)
        n = tensor.numel()
        return error_report(n, [n * 0.5, n * 0.25, n * 4.0, 0.75, 0.0])

    args = verify.parse_args(["--model_id", src, "--quantized_dir", str(out), "--log_level", "ERROR", "--worst", "1"])
    assert verify.verify(args, error_fn=stub) == 0
    assert set(seen) == {(4, 256), (2, 128)}
    assert all(("qweight" in keys) == packed for keys in seen.values())
    rep = json.load(open(out / "quantization_error.json"))
    assert set(rep["tensors"]) == set(tensors) and rep["problems"] == {}
    e = rep["tensors"]["a.weight"]
    assert (e["numel"], e["nonfinite"], e["mean_abs_error"], e["mse"], e["max_abs_error"]) == (1024, 0, 0.5, 0.25, 0.75)
    assert e["snr_db"] == 10.0 * math.log10(16.0)
    t = rep["totals"]
    assert (t["tensors"], t["numel"], t["sum_abs"], t["mean_abs_error"], t["max_abs_error"]) == (2, 1280, 640.0, 0.5, 0.75)


def test_verify_returns_1_for_missing_source_shape_mismatch_and_autoawq(tmp_path):
    from safetensors.torch import save_file
    from awq_quantizer import verify
    from awq_quantizer.main import save_model_in_chunks
    from awq_quantizer.quantization.awq import error_report
    src, tensors = _write_model(tmp_path)
    res = _fake_results(tensors, packed=True)
    res["c.weight"] = res["a.weight"]                                     # no source of this name
    res["b.weight"] = dict(res["b.weight"], shape=torch.tensor([128, 2]))   # shape disagrees
    out = tmp_path / "out"
    save_model_in_chunks(res, str(out), chunk_size=10)
    report = tmp_path / "reports" / "r.json"
    args = verify.parse_args(["--model_id", src, "--quantized_dir", str(out), "--report", str(report),
                              "--log_level", "CRITICAL"])
    assert verify.verify(args, error_fn=lambda t, r: error_report(t.numel(), [1.0, 1.0, 1.0, 1.0, 0.0])) == 1
    rep = json.load(open(report))
    assert set(rep["tensors"]) == {"a.weight"} and set(rep["problems"]) == {"b.weight", "c.weight"}
    # an AutoAWQ-layout directory has no metadata.json: out of scope, reported as such
    auto = tmp_path / "auto"
    auto.mkdir()
    save_file({"x.qweight": torch.zeros(4, dtype=torch.int32)}, str(auto / "model.safetensors"))
    args = verify.parse_args(["--model_id", src, "--quantized_dir", str(auto), "--log_level", "CRITICAL"])
    assert verify.verify(args, error_fn=lambda t, r: None) == 1
    with pytest.raises(FileNotFoundError, match="autoawq"):
        next(verify.iter_results(str(auto)))
    args = verify.parse_args(["--model_id", str(tmp_path / "nope"), "--quantized_dir", str(out), "--log_level",
                              "CRITICAL"])
    assert verify.verify(args, error_fn=lambda t, r: None) == 1


def test_verify_passes_input_scale_on_and_marks_the_entry(tmp_path):
    """Results of --scale_method awq --act_stats carry input_scale (they quantize W * diag(s)): the
    chunk loads, the error function receives the key, and the entry says it was measured scaled."""
    from awq_quantizer import verify
    from awq_quantizer.main import save_model_in_chunks
    from awq_quantizer.quantization.awq import error_report
    src, tensors = _write_model(tmp_path)
    for st in (False, True):
        res = _fake_results(tensors, packed=True)
        res["a.weight"]["input_scale"] = torch.full((256,), 2.0)
        out = tmp_path / f"out{int(st)}"
        save_model_in_chunks(res, str(out), chunk_size=10, use_safetensors=st)
        seen = {}

        def stub(tensor, result):
            seen[tuple(tensor.shape)] = result.get("input_scale")
            return error_report(tensor.numel(), [1.0, 1.0, 4.0, 1.0, 0.0])

        args = verify.parse_args(["--model_id", src, "--quantized_dir", str(out), "--log_level", "ERROR"])
        assert verify.verify(args, error_fn=stub) == 0
        assert torch.equal(seen[(4, 256)], torch.full((256,), 2.0)) and seen[(2, 128)] is None
        rep = json.load(open(out / "quantization_error.json"))
        assert rep["tensors"]["a.weight"]["input_scaled"] is True
        assert rep["tensors"]["b.weight"]["input_scaled"] is False


def test_quantization_error_rejects_a_mismatched_input_scale():
    q = _quantizer()
    x = torch.randn(2, 256)
    res = {"qweight": torch.zeros((2, 32), dtype=torch.int32), "qzeros": torch.zeros((2, 1), dtype=torch.int32),
           "scales": torch.ones((2, 2), dtype=torch.float16), "bits": torch.tensor(4, dtype=torch.int32),
           "group_size": torch.tensor(128, dtype=torch.int32), "symmetric": torch.tensor(False),
           "shape": torch.tensor([2, 256]), "input_scale": torch.ones(128)}
    with pytest.raises(ValueError, match="input_scale"):
        q.quantization_error(x, res)


def test_worst_tensors_order():
    """Tensors with no finite element first (their snr_db reads inf: sum_sq is 0), then ascending snr_db."""
    from awq_quantizer import verify
    from awq_quantizer.quantization.awq import error_report
    entries = {"good": error_report(8, [1.0, 0.01, 100.0, 0.5, 0.0]),       # 40 dB
               "bad": error_report(8, [1.0, 10.0, 100.0, 0.5, 1.0]),        # 10 dB
               "exact": error_report(8, [0.0, 0.0, 100.0, 0.0, 0.0]),       # inf
               "zero_source": error_report(8, [1.0, 1.0, 0.0, 0.5, 0.0]),   # -inf
               "nothing_finite": error_report(8, [0.0, 0.0, 0.0, 0.0, 8.0])}
    assert entries["zero_source"]["snr_db"] == -math.inf and entries["nothing_finite"]["snr_db"] == math.inf
    assert verify.worst_tensors(entries, 5) == ["nothing_finite", "zero_source", "bad", "good", "exact"]
    assert verify.worst_tensors(entries, 2) == ["nothing_finite", "zero_source"]
    assert verify.worst_tensors(entries, 0) == []
