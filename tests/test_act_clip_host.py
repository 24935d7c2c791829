"""Activation-aware clip search, the parts that need no GPU: argument validation of
awq_quantize_clip_scaled (everything is checked before a launch), the --act_clip flags and their
misuse errors, and quantize_layer_group's argument errors."""
import ctypes

import pytest
import torch
from safetensors.torch import save_file

P = ctypes.c_void_p(4096)      # a non-null, 16-B aligned address that is never dereferenced


def _call(**kw):
    from awq_quantizer import _hip
    a = dict(w=P, dtype=0, rows=8, K=256, gs=128, bits=4, sym=0, cs=P, rs=None, xs=P, n_grid=20, n_cand=10, qweight=P,
             qzeros=P, scales=P, best=None, loss=None, stride=0)
    a.update(kw)
    rc = _hip.load_library().awq_quantize_clip_scaled(
        a["w"], a["dtype"], a["rows"], a["K"], a["gs"], a["bits"], a["sym"], a["cs"], a["rs"], a["xs"], a["n_grid"],
        a["n_cand"], a["qweight"], a["qzeros"], a["scales"], a["best"], a["loss"], a["stride"], None)
    return rc, _hip.last_error()


def test_binding_and_abi():
    from awq_quantizer import _hip
    lib = _hip.load_library()
    assert hasattr(lib, "awq_quantize_clip_scaled") and "awq_quantize_clip_scaled" in _hip.SIGNATURES
    assert lib.awq_abi_version() == 17
    assert callable(_hip.quantize_clip_scaled)


@pytest.mark.parametrize("kw,code,word", [
    (dict(w=None), 1, "null input"),
    (dict(cs=None), 1, "null input"),
    (dict(xs=None), 1, "null input"),
    (dict(n_cand=21), 1, "n_candidates"),
    (dict(n_cand=0), 1, "n_candidates"),
    (dict(n_grid=0, n_cand=0), 1, "n_grid"),
    (dict(qweight=None, qzeros=None, scales=None), 1, "no output requested"),
    (dict(dtype=9), 1, "dtype"),
    (dict(dtype=-1), 1, "dtype"),
    (dict(dtype=3), 2, "fp64"),
    (dict(bits=3), 1, "bit width"),
    (dict(gs=0), 1, "Group size"),
    (dict(rows=-1), 1, "negative shape"),
    (dict(gs=96, K=384), 2, "power of two"),
    (dict(gs=1024, K=2048), 2, "512"),
    (dict(gs=4, K=256), 2, "power of two"),
    (dict(K=320), 2, "dividing K"),
    (dict(loss=P, stride=15), 1, "loss_stride"),
    (dict(w=ctypes.c_void_p(4097)), 1, "aligned"),
    (dict(cs=ctypes.c_void_p(4098)), 1, "aligned"),
    (dict(scales=ctypes.c_void_p(4097)), 1, "aligned"),
])
def test_invalid_arguments_are_reported_before_any_launch(kw, code, word):
    rc, msg = _call(**kw)
    assert rc == code and word in msg, (rc, msg)


def test_empty_tensor_and_single_outputs_are_fine():
    assert _call(rows=0) == (0, "")
    # best_idx or group_loss alone counts as an output (validation then passes; nothing to launch)
    assert _call(rows=0, qweight=None, qzeros=None, scales=None, best=P)[0] == 0
    assert _call(rows=0, qweight=None, qzeros=None, scales=None, loss=P, stride=16)[0] == 0


def test_python_wrapper_checks_the_loss_buffer():
    from awq_quantizer import _hip
    w = torch.zeros(2, 256, dtype=torch.bfloat16)
    v = torch.ones(256)
    for bad in (torch.zeros(2, 3), torch.zeros(3, 4), torch.zeros(2, 4, dtype=torch.float64)):
        with pytest.raises(ValueError, match="group_loss"):
            _hip.quantize_clip_scaled(w, v, v, 128, 4, False, 20, 10, group_loss=bad)
    with pytest.raises(ValueError, match="group_loss"):
        _hip.quantize_clip_scaled(w, v, v, 128, 4, False, 20, 10, group_loss=torch.zeros(2, 4), loss_offset=1)


def test_cli_flags_parse():
    from awq_quantizer.main import parse_args
    a = parse_args(["--model_id", "m", "--output_dir", "o"])
    assert (a.act_clip, a.clip_grid, a.clip_max_shrink) == (False, 20, 0.5)
    a = parse_args(["--model_id", "m", "--output_dir", "o", "--scale_method", "awq", "--act_stats", "s.st",
                    "--act_clip", "--clip_grid", "16", "--clip_max_shrink", "0.25"])
    assert (a.act_clip, a.clip_grid, a.clip_max_shrink) == (True, 16, 0.25)


def test_cli_act_clip_misuse_is_an_error(tmp_path):
    from awq_quantizer.main import main
    src = tmp_path / "model"
    src.mkdir()
    save_file({"a.weight": torch.zeros(4, 128, dtype=torch.bfloat16)}, str(src / "model.safetensors"))
    stats = str(tmp_path / "stats.safetensors")
    save_file({"a.weight.x_mean": torch.ones(128), "a.weight.x_sq": torch.ones(128)}, stats)
    base = ["--model_id", str(src), "--log_level", "CRITICAL", "--act_clip"]
    awq = ["--scale_method", "awq", "--act_stats", stats]
    # without the activation-aware search there is nothing to clip against
    assert main(base + ["--output_dir", str(tmp_path / "o1")]) == 1
    assert main(base + ["--output_dir", str(tmp_path / "o2"), "--scale_method", "awq"]) == 1
    assert main(base + ["--output_dir", str(tmp_path / "o3"), "--scale_method", "search"]) == 1
    # the kernel writes packed outputs only
    assert main(base + awq + ["--output_dir", str(tmp_path / "o4")]) == 1
    assert main(base + awq + ["--output_dir", str(tmp_path / "o5"), "--output_format", "reference"]) == 1
    # grid values
    assert main(base + awq + ["--output_dir", str(tmp_path / "o6"), "--output_format", "packed", "--clip_grid",
                              "0"]) == 1
    assert main(base + awq + ["--output_dir", str(tmp_path / "o7"), "--output_format", "packed",
                              "--clip_max_shrink", "1.5"]) == 1
    for k in range(1, 8):       # every one of them stopped before any output was written
        d = tmp_path / f"o{k}"
        assert not d.exists() or not any(d.iterdir())


def test_layer_group_clip_argument_errors():
    from awq_quantizer.quantization import AWQQuantizer
    w = {"a": torch.zeros(4, 256, dtype=torch.bfloat16)}
    v = torch.ones(256)
    q = AWQQuantizer(bits=4, group_size=128, symmetric=False, scale_method="awq", device="cuda:0",
                     logger_level="CRITICAL")
    with pytest.raises(ValueError, match="packed"):
        q.quantize_layer_group(w, x_mean=v, x_sq=v, packed=False, clip=True)
    with pytest.raises(ValueError, match="clip_grid"):
        q.quantize_layer_group(w, x_mean=v, x_sq=v, clip=True, clip_grid=0)
    with pytest.raises(ValueError, match="clip_grid"):
        q.quantize_layer_group(w, x_mean=v, x_sq=v, clip=True, clip_grid=2.5)
    with pytest.raises(ValueError, match="clip_max_shrink"):
        q.quantize_layer_group(w, x_mean=v, x_sq=v, clip=True, clip_max_shrink=1.5)
    rtn = AWQQuantizer(bits=4, group_size=128, symmetric=False, device="cuda:0", logger_level="CRITICAL")
    with pytest.raises(ValueError, match="scale_method"):
        rtn.quantize_layer_group(w, x_mean=v, x_sq=v, clip=True)
