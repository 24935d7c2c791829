"""Activation-aware MXFP4 without a GPU: --mxfp4_act_scales' option rules, each with its own
message and nothing launched, and what the two entries and the Python layer refuse before the device is
touched, in awq_quantize_mxfp4's order."""
import pytest
import torch

BASE = ["--model_id", "m", "--output_dir", "o"]


@pytest.mark.parametrize("extra,message", [
    (["--output_format", "packed", "--mxfp4_act_scales", "--act_stats", "s"], "MXFP4_ACT_NEEDS"),
    (["--output_format", "mxfp4", "--mxfp4_act_scales"], "MXFP4_ACT_STATS"),
    (["--output_format", "mxfp4", "--mxfp4_act_scales", "--act_stats", "s", "--mxfp4_rounding", "gptq",
      "--act_samples", "x"], "MXFP4_ACT_NO_GPTQ"),
])
def test_refused_combinations(extra, message, monkeypatch, tmp_path):
    from awq_quantizer import _hip, main as cli, options
    assert options.check_args(options.parse_args(BASE + extra), 1, 1, None) == getattr(options, message)
    monkeypatch.setattr(_hip, "load_library", lambda *a, **k: pytest.fail("the library was loaded"))
    monkeypatch.setattr(cli, "load_model_from_hub", lambda *a, **k: pytest.fail("the model was read"))
    argv = BASE[:3] + [str(tmp_path / "out")] + extra
    assert cli.main(argv + ["--device", "cpu", "--log_level", "CRITICAL"]) == 1


def test_accepted_with_statistics():
    from awq_quantizer import options
    args = options.parse_args(BASE + ["--output_format", "mxfp4", "--mxfp4_act_scales", "--act_stats", "s"])
    assert options.check_args(args, 1, 1, "llama") is None


# (dtype, rows, K, rule, n_grid) -> a word of the message; the last: nothing wrong but the pointers
CASES = [((0, 4, 48, 0, 2), "K % 32"), ((3, 4, 64, 0, 2), "dtype"), ((0, 4, 64, 7, 2), "rule"),
         ((0, -1, 64, 0, 2), "negative"), ((0, 1 << 31, 1 << 31, 0, 2), "2^60"), ((0, 4, 64, 0, 2), "null")]


@pytest.mark.parametrize("args,word", CASES + [((0, 4, 64, 0, 0), "n_grid"), ((0, 4, 64, 0, 257), "n_grid")])
def test_entries_refuse(args, word):
    from awq_quantizer import _hip
    dtype, rows, K, rule, n_grid = args
    lib = _hip.load_library()
    assert lib.awq_act_search_losses_mxfp4(None, dtype, rows, K, rule, None, None, n_grid, None, None, rows * (K // 32),
                                           None) != 0
    assert word in _hip.last_error()
    if word != "n_grid":
        assert lib.awq_quantize_mxfp4_scaled(None, dtype, rows, K, rule, None, None, None, None) != 0
        assert word in _hip.last_error()


def test_empty_problems_look_at_no_pointer():
    from awq_quantizer import _hip
    lib = _hip.load_library()
    assert lib.awq_act_search_losses_mxfp4(None, 0, 0, 64, 0, None, None, 2, None, None, 0, None) == 0
    assert lib.awq_quantize_mxfp4_scaled(None, 1, 4, 0, 2, None, None, None, None) == 0
    assert lib.awq_act_search_losses_mxfp4(None, 0, 4, 64, 0, None, None, 2, None, None, 7, None) != 0
    assert "part_stride" in _hip.last_error()


def test_python_layer_refuses_before_the_device():
    from awq_quantizer.quantization import act_mxfp4
    for bad in (torch.zeros(4, 48), torch.zeros(64), torch.zeros(4, 64, dtype=torch.float64)):
        with pytest.raises(ValueError):
            act_mxfp4.quantize_layer_group_mxfp4(None, {"w": bad}, x_mean=torch.ones(64), x_sq=torch.ones(64))
    with pytest.raises(ValueError, match="scale_rule"):
        act_mxfp4.quantize_layer_group_mxfp4(None, {"w": torch.zeros(4, 64)}, scale_rule="nearest")
