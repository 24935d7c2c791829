"""awq_mxfp4_gemm without a GPU: the symbol in both libraries and the binding, the entry's
refusals with their messages before any pointer is followed, and evaluate's --mxfp4_activations rule."""
import ctypes
import json

import pytest

FAKE = ctypes.c_void_p(4096)          # never followed: every case below fails before a launch
ODD = ctypes.c_void_p(4098)


def call(lib, T=4, N=4, K=64, a=FAKE, w=FAKE, s=FAKE, bias=None, bias_dtype=0, out=FAKE, out_dtype=2):
    return lib.awq_mxfp4_gemm(a, s, T, w, s, N, K, bias, bias_dtype, out, out_dtype, None)


def test_symbol_is_exported_and_bound():
    from awq_quantizer import _hip
    assert "awq_mxfp4_gemm" in _hip.SIGNATURES
    for lib in (_hip.load_library(), ctypes.CDLL(_hip.DIAG_LIB_PATH)):
        assert lib.awq_mxfp4_gemm is not None
    assert _hip.load_library().awq_abi_version() == 17


@pytest.mark.parametrize("kw,word", [
    (dict(T=0), "positive"), (dict(N=-1), "positive"), (dict(K=0), "positive"), (dict(K=48), "K % 32"),
    (dict(out_dtype=3), "out dtype"), (dict(bias=FAKE, bias_dtype=7), "bias dtype"),
    (dict(T=1 << 31, K=1 << 31), "2^60"), (dict(a=None), "null"), (dict(s=None), "null"), (dict(out=None), "null"),
    (dict(a=ODD), "alignment"), (dict(out=ODD), "alignment"), (dict(bias=ODD, bias_dtype=2), "alignment"),
])
def test_entry_refuses(kw, word):
    from awq_quantizer import _hip
    assert call(_hip.load_library(), **kw) != 0
    assert word in _hip.last_error()


def test_evaluate_refuses_the_flag_without_an_mxfp4_directory(tmp_path):
    from awq_quantizer import evaluate
    src, other = tmp_path / "src", tmp_path / "other"
    src.mkdir()
    other.mkdir()
    (other / "model.safetensors").write_bytes(b"")
    (other / "quant_config.json").write_text(json.dumps({"w_bit": 4, "q_group_size": 128, "zero_point": True,
                                                         "version": "gemm"}))
    base = ["--model_id", str(src), "--input_ids", "ids", "--mxfp4_activations"]
    for extra in ([], ["--quantized_dir", str(other)]):
        assert evaluate.check_args(evaluate.build_parser().parse_args(base + extra)) == evaluate.MXFP4_ACT_NEEDS
    (other / "config.json").write_text(json.dumps({"quantization_config": {"quant_method": "mxfp4", "block_size": 32}}))
    args = evaluate.build_parser().parse_args(base + ["--quantized_dir", str(other)])
    assert evaluate.check_args(args) is None
    assert "float16" in evaluate.check_args(evaluate.build_parser().parse_args(
        base + ["--quantized_dir", str(other), "--compute_dtype", "float16"]))
    assert evaluate.main(base + ["--log_level", "CRITICAL"]) == 1
