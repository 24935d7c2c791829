"""MXFP4 without a GPU: the option rules of --output_format mxfp4 — every refused
combination gives its own message with nothing launched — and what the entries and the Python layer
refuse before the device is touched."""
import pytest
import torch

BASE = ["--model_id", "m", "--output_dir", "o", "--output_format", "mxfp4"]


@pytest.mark.parametrize("extra,world,message", [
    ([], 2, "MXFP4_ONE_PROCESS"),
    (["--scale_method", "search"], 1, "MXFP4_SCALE_METHOD"),
    (["--scale_method", "awq"], 1, "MXFP4_SCALE_METHOD"),
    (["--scale_method", "awq", "--act_stats", "s", "--fold_scales"], 1, "MXFP4_SCALE_METHOD"),
    (["--fold_scales"], 1, "MXFP4_NO_FOLD"),
    (["--act_clip"], 1, "MXFP4_NO_CLIP"),
    (["--rounding", "gptq"], 1, "MXFP4_NO_GPTQ"),
    (["--bits", "8"], 1, "MXFP4_BITS"),
])
def test_refused_combinations(extra, world, message, monkeypatch, tmp_path):
    from awq_quantizer import _hip, main as cli, options
    want = getattr(options, message)
    assert options.check_args(options.parse_args(BASE + extra), world, 1, None) == want
    if world == 1:      # the CLI itself: the message is logged and nothing is loaded or launched
        monkeypatch.setattr(_hip, "load_library", lambda *a, **k: pytest.fail("the library was loaded"))
        monkeypatch.setattr(cli, "load_model_from_hub", lambda *a, **k: pytest.fail("the model was read"))
        argv = BASE[:3] + [str(tmp_path / "out")] + BASE[4:] + extra
        assert cli.main(argv + ["--device", "cpu", "--log_level", "CRITICAL"]) == 1


def test_accepted_flags():
    from awq_quantizer import options
    for extra in ([], ["--mxfp4_scale", "ceil"], ["--mxfp4_scale", "mse", "--scale_method", "minmax"]):
        assert options.check_args(options.parse_args(BASE + extra), 1, 1, None) is None
    other = options.parse_args(BASE[:4] + ["--output_format", "packed", "--mxfp4_scale", "mse"])
    assert options.check_args(other, 1, 1, None) == options.MXFP4_SCALE_NEEDS
    with pytest.raises(SystemExit):
        options.parse_args(BASE + ["--mxfp4_scale", "nearest"])


@pytest.mark.parametrize("args,word", [((0, 4, 48, 0), "K % 32"), ((3, 4, 64, 0), "dtype"), ((0, 4, 64, 7), "rule"),
                                       ((0, -1, 64, 0), "negative"), ((0, 4, 64, 0), "null")])
def test_entry_refuses(args, word):
    from awq_quantizer import _hip
    dtype, rows, K, rule = args
    assert _hip.load_library().awq_quantize_mxfp4(None, dtype, rows, K, rule, None, None, None) != 0
    assert word in _hip.last_error()


def test_python_layer_refuses_before_the_device():
    from awq_quantizer.quantization import mxfp4
    for bad in (torch.zeros(4, 48), torch.zeros(64), torch.zeros(4, 64, dtype=torch.float64)):
        with pytest.raises(ValueError):
            mxfp4.quantize_mxfp4(None, bad)
    with pytest.raises(ValueError, match="scale_rule"):
        mxfp4.quantize_mxfp4(None, torch.zeros(4, 64), "nearest")
    with pytest.raises(ValueError, match="per_group"):
        mxfp4.quantization_error(None, torch.zeros(4, 64), {"format": "mxfp4"}, per_group=True)
