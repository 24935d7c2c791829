"""GPTQ-compensated MXFP4 without a GPU: the option rules of --mxfp4_rounding — every
refused combination gives its own message with nothing launched — and what the entry and the Python
layer refuse before the device is touched."""
import pytest
import torch

BASE = ["--model_id", "m", "--output_dir", "o", "--output_format", "mxfp4"]
GPTQ = ["--mxfp4_rounding", "gptq"]


@pytest.mark.parametrize("argv,message", [
    (BASE + GPTQ, "MXFP4_GPTQ_SAMPLES"),
    (BASE[:4] + ["--output_format", "packed", "--mxfp4_rounding", "nearest"], "MXFP4_ROUNDING_NEEDS"),
    (BASE[:4] + ["--output_format", "packed"] + GPTQ, "MXFP4_ROUNDING_NEEDS"),
    (BASE + GPTQ + ["--act_samples", "s", "--rounding", "gptq"], "MXFP4_NO_GPTQ"),
    (BASE + GPTQ + ["--act_samples", "s", "--gptq_damp", "1.5"], "--gptq_damp must be in (0, 1)"),
    (BASE + ["--act_samples", "s"], "--act_samples is read by --search_loss output"),
    (BASE + ["--gptq_factor", "hip"], "--gptq_factor is read by --rounding gptq"),
])
def test_refused_combinations(argv, message, monkeypatch, tmp_path):
    from awq_quantizer import _hip, main as cli, options
    want = getattr(options, message, message)
    assert options.check_args(options.parse_args(argv), 1, 1, None) == want
    monkeypatch.setattr(_hip, "load_library", lambda *a, **k: pytest.fail("the library was loaded"))
    monkeypatch.setattr(cli, "load_model_from_hub", lambda *a, **k: pytest.fail("the model was read"))
    argv = argv[:3] + [str(tmp_path / "out")] + argv[4:]
    assert cli.main(argv + ["--device", "cpu", "--log_level", "CRITICAL"]) == 1


def test_accepted_flags():
    from awq_quantizer import options
    for extra in (["--mxfp4_rounding", "nearest"], GPTQ + ["--act_samples", "s"],
                  GPTQ + ["--act_samples", "s", "--gptq_factor", "hip", "--gptq_damp", "0.05", "--mxfp4_scale", "mse"]):
        args = options.parse_args(BASE + extra)
        assert options.check_args(args, 1, 1, None) is None
        assert options.wants_samples(args) == ("gptq" in extra)
    with pytest.raises(SystemExit):
        options.parse_args(BASE + ["--mxfp4_rounding", "floor"])


@pytest.mark.parametrize("args,word", [((4, 48, 0, 0, 32), "K % 32"), ((4, 256, 0, 0, 160), "n_cols"),
                                       ((4, 256, 0, 16, 32), "col_begin"), ((4, 256, 7, 0, 128), "rule"),
                                       ((-1, 256, 0, 0, 128), "negative"), ((4, 256, 0, 0, 128), "null")])
def test_entry_refuses(args, word):
    from awq_quantizer import _hip
    N, K, rule, c0, n = args
    assert _hip.load_library().awq_gptq_round_block_mxfp4(None, N, K, rule, None, c0, n, None, None, None, None) != 0
    assert word in _hip.last_error()


def test_python_layer_refuses_before_the_device():
    from awq_quantizer.quantization import gptq_mxfp4
    w, x = torch.zeros(4, 64), torch.zeros(8, 64)
    for bad in (torch.zeros(4, 48), torch.zeros(64), torch.zeros(4, 64, dtype=torch.float64)):
        with pytest.raises(ValueError):
            gptq_mxfp4.quantize_gptq_mxfp4(None, bad, x)
    for kw, match in (({"scale_rule": "nearest"}, "scale_rule"), ({"damp": 1.0}, "damp"), ({"damp": True}, "damp"),
                      ({"samples": torch.zeros(8, 32)}, "samples"), ({"hessian": torch.zeros(32, 32)}, "hessian"),
                      ({}, "needs token samples")):
        with pytest.raises(ValueError, match=match):
            gptq_mxfp4.quantize_gptq_mxfp4(None, w, **kw)
