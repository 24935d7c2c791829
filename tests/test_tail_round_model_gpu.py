"""--rounding gptq from the calibration pass to a written checkpoint, on the committed
tests/golden/model_llama fixture: main --fold_scales --calib_ids --rounding gptq for
--output_format autoawq and for --output_format gptq --symmetric, beside the same runs with
--rounding nearest; the checkpoints read back by tests/checkpoint_reader.py / tests/gptq_reader.py
and tests/model_forward.py, and measured by verify --act_samples.

Measured on an MI355X (llama bf16, group size 32, 128 calibration tokens, all kept as samples):
  autoawq:        e_textbook 6.181e-03; nearest e / e_textbook 0.735, gptq 0.572; summed logged output
                  error compensated / nearest 0.4016; verify --act_samples 148.16 -> 59.5062
  gptq symmetric: nearest e / e_textbook 0.980, gptq 0.845; summed logged output error 0.4443;
                  verify --act_samples 447.989 -> 199.047
No ordering of the two roundings' logit errors is asserted: a 2-block model and 128 tokens do not
carry one.  Asserted: the scale search is untouched (awq_scales.safetensors byte for byte), the
model bytes differ, every weight's logged output error does not grow, verify accepts all four
directories and reports a smaller total output error for the compensated run, and the asymmetric
checkpoints' logit error stays inside THETA * e_textbook (the textbook reference is asymmetric).
Each CLI run is made once per module."""
import json
import os
import re

import pytest
import torch
from safetensors.torch import save_file

import model_cases as mc
from checkpoint_reader import read_checkpoint
from gptq_reader import read_gptq
from test_gpu_calibrate import calib_ids

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]

TOKENS = 128           # calib_ids: 4 sequences of 32 tokens, all kept
LINE = re.compile(r"(\S+\.weight): gptq rounding, output error (\S+) -> (\S+?)(?: \(fallback: nearest\))?$", re.M)
LAYOUTS = {"autoawq": [], "gptq": ["--symmetric"]}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from awq_quantizer import _hip, calibrate
    from awq_quantizer.main import main
    _hip.require_device(torch.device("cuda", 0))
    fx = mc.fixture("llama")
    root = tmp_path_factory.mktemp("round_model")
    model = root / "model"
    model.mkdir()
    save_file(dict(fx.state), str(model / "model.safetensors"), metadata={"format": "pt"})
    with open(model / "config.json", "w") as f:
        json.dump(fx.config, f)
    ids = str(root / "ids.safetensors")
    save_file({"input_ids": calib_ids("llama")}, ids)
    smp = str(root / "samples.safetensors")
    assert calibrate.main(["--model_id", str(model), "--output", str(root / "stats.safetensors"), "--input_ids", ids,
                           "--device", "cuda:0", "--compute_dtype", "bfloat16", "--samples_output", smp,
                           "--n_sample_tokens", str(TOKENS), "--log_level", "ERROR"]) == 0
    out, log = {}, {}
    for layout, extra in LAYOUTS.items():
        for rounding in ("nearest", "gptq"):
            k = (layout, rounding)
            out[k], log[k] = str(root / f"{layout}_{rounding}"), str(root / f"{layout}_{rounding}.log")
            assert main(["--model_id", str(model), "--group_size", "32", "--device", "cuda:0", "--output_format", layout,
                         "--scale_method", "awq", "--fold_scales", "--calib_ids", ids, "--n_sample_tokens", str(TOKENS),
                         "--rounding", rounding, "--output_dir", out[k], "--log_file", log[k]] + extra) == 0
    return {"fx": fx, "root": root, "model": str(model), "samples": smp, "out": out, "log": log}


def _data(d, f="model.safetensors"):
    return open(os.path.join(d, f), "rb").read()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_checkpoints(runs, layout):
    fx, out = runs["fx"], runs["out"]
    near, comp = out[(layout, "nearest")], out[(layout, "gptq")]
    assert _data(near, "awq_scales.safetensors") == _data(comp, "awq_scales.safetensors")     # the same scale search
    assert _data(near) != _data(comp)
    read = read_gptq if layout == "gptq" else read_checkpoint
    states = {}
    for k, d in (("nearest", near), ("gptq", comp)):
        states[k], info = read(d)
        assert {n: tuple(t.shape) for n, t in states[k].items()} == fx.names
        assert set(info["quantized"]) == set(fx.quantized_names("autoawq"))
    lines = LINE.findall(open(runs["log"][(layout, "gptq")]).read())
    assert {m for m, _, _ in lines} == set(fx.quantized_names("autoawq")) and len(lines) == len(fx.quantized_names("autoawq"))
    for m, before, after in lines:
        assert float(after) <= float(before), (m, before, after)
    assert "fallback: nearest" not in open(runs["log"][(layout, "gptq")]).read()
    assert not LINE.findall(open(runs["log"][(layout, "nearest")]).read())
    ratio = sum(float(a) for _, _, a in lines) / sum(float(b) for _, b, _ in lines)
    e = {k: fx.e(s) for k, s in states.items()}
    et = mc.e_textbook("llama", "autoawq", 32)
    print(f"rounding llama bf16 gs32 {layout}{' sym' if layout == 'gptq' else ''}: e_textbook {et:.3e}  nearest "
          f"e/e_textbook {e['nearest'] / et:.3f}  gptq e/e_textbook {e['gptq'] / et:.3f}; summed logged output error "
          f"compensated / nearest {ratio:.4f}")
    if layout == "autoawq":
        assert e["gptq"] < mc.THETA * et and e["nearest"] < mc.THETA * et


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_verify_reports_a_smaller_output_error(runs, layout):
    from awq_quantizer import verify
    total = {}
    for rounding in ("nearest", "gptq"):
        report = str(runs["root"] / f"report_{layout}_{rounding}.json")
        assert verify.main(["--model_id", runs["model"], "--quantized_dir", runs["out"][(layout, rounding)],
                            "--act_samples", runs["samples"], "--report", report, "--device", "cuda:0",
                            "--log_level", "ERROR"]) == 0
        rep = json.load(open(report))
        assert rep["problems"] == {} and set(rep["tensors"]) == set(runs["fx"].quantized_names("autoawq"))
        assert rep["totals"]["output_tensors"] == len(rep["tensors"])
        total[rounding] = rep["totals"]["output_sum_sq"]
    print(f"verify --act_samples {layout}: total output error nearest {total['nearest']:.6g}  gptq {total['gptq']:.6g}  "
          f"ratio {total['gptq'] / total['nearest']:.4f}")
    assert total["gptq"] < total["nearest"]
