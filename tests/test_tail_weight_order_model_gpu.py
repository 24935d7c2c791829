"""--gptq_act_order from the calibration pass to a written, verified and evaluated checkpoint, on the
committed tests/golden/model_llama fixture, as tests/test_tail_round_model_gpu.py
does for --rounding gptq: one main run with act-order and one without.  The summed output errors
(act-order / in-order / nearest) are printed, not ordered: a 2-block model does not carry one."""
import json

import pytest
import torch
from safetensors.torch import save_file

import model_cases as mc
from gptq_reader import read_gptq
from test_gpu_calibrate import calib_ids
from test_tail_round_model_gpu import LINE, TOKENS

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]
GS = 32


def test_act_order_checkpoint_round_trip(tmp_path):
    from awq_quantizer import _hip, calibrate, evaluate, verify
    from awq_quantizer.main import main
    from awq_quantizer.quantization import AWQQuantizer
    _hip.require_device(torch.device("cuda", 0))
    fx = mc.fixture("llama")
    model = tmp_path / "model"
    model.mkdir()
    save_file(dict(fx.state), str(model / "model.safetensors"), metadata={"format": "pt"})
    (model / "config.json").write_text(json.dumps(fx.config))
    ids, smp = str(tmp_path / "ids.safetensors"), str(tmp_path / "samples.safetensors")
    save_file({"input_ids": calib_ids("llama")}, ids)
    assert calibrate.main(["--model_id", str(model), "--output", str(tmp_path / "stats.safetensors"), "--input_ids", ids,
                           "--device", "cuda:0", "--compute_dtype", "bfloat16", "--samples_output", smp,
                           "--n_sample_tokens", str(TOKENS), "--log_level", "ERROR"]) == 0
    sums = {}
    for name, extra in (("act", ["--gptq_act_order"]), ("in", [])):
        out, log = str(tmp_path / name), str(tmp_path / f"{name}.log")
        assert main(["--model_id", str(model), "--group_size", str(GS), "--device", "cuda:0", "--output_format", "gptq",
                     "--scale_method", "awq", "--fold_scales", "--calib_ids", ids, "--n_sample_tokens", str(TOKENS),
                     "--rounding", "gptq", "--output_dir", out, "--log_file", log] + extra) == 0
        lines = LINE.findall(open(log).read())
        assert len(lines) == len(fx.quantized_names("autoawq")) and "fallback: nearest" not in open(log).read()
        sums[name], sums["nearest"] = sum(float(a) for _, _, a in lines), sum(float(b) for _, b, _ in lines)
        for cfg in (json.load(open(out + "/quantize_config.json")), json.load(open(out + "/config.json"))["quantization_config"]):
            assert cfg["desc_act"] is (name == "act")
    print(f"summed output error llama bf16 gs{GS}: act-order {sums['act']:.6g}  in-order {sums['in']:.6g}  "
          f"nearest {sums['nearest']:.6g}")
    out = str(tmp_path / "act")
    state, info = read_gptq(out)
    assert set(info["quantized"]) == set(fx.quantized_names("autoawq"))
    q = AWQQuantizer(bits=4, group_size=GS, device="cuda:0", logger_level="ERROR")
    for name, p in info["quantized"].items():
        g, K = p["g_idx"].long(), p["g_idx"].numel()
        assert bool((torch.bincount(g, minlength=K // GS) == GS).all()) and not torch.equal(g, torch.arange(K) // GS), name
        got = q.dequantize_gptq(p, checkpoint_format=info["quantize_config"]["checkpoint_format"]).cpu()
        assert torch.equal(got, state[name].half().float()), name      # (the reader's float64 product, rounded once)
    report = str(tmp_path / "report.json")
    assert verify.main(["--model_id", str(model), "--quantized_dir", out, "--act_samples", smp, "--report", report,
                        "--device", "cuda:0", "--log_level", "ERROR"]) == 0
    rep = json.load(open(report))
    assert rep["problems"] == {} and set(rep["tensors"]) == set(info["quantized"])
    assert evaluate.main(["--model_id", str(model), "--quantized_dir", out, "--input_ids", ids, "--device", "cuda:0",
                          "--log_level", "ERROR"]) == 0
