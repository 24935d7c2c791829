"""--output_format mxfp4 --mxfp4_rounding gptq end to end on the llama fixture: main writes
the directory from calibrate's samples, verify returns 0, config.json records the rounding, lm_head (no
samples) keeps the nearest run's bytes, and the output error on the samples, summed over the grouped
linears, is below the nearest directory's."""
import json

import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

import model_cases as mc
import mxfp4_ref as ref
from test_gpu_calibrate import calib_ids

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]


def test_gptq_directory(tmp_path):
    from awq_quantizer import calibrate, verify
    from awq_quantizer.main import main
    from awq_quantizer.mxfp4_cli import sample_keys
    from awq_quantizer.model_loading.safetensors_loader import SafetensorsLoader
    fx, src = mc.fixture("llama"), tmp_path / "src"
    src.mkdir()
    save_file(dict(fx.state), str(src / "model.safetensors"), metadata={"format": "pt"})
    (src / "config.json").write_text(json.dumps(fx.config))
    ids, smp = str(tmp_path / "ids.safetensors"), str(tmp_path / "samples.safetensors")
    save_file({"input_ids": calib_ids("llama")}, ids)
    assert calibrate.main(["--model_id", str(src), "--output", str(tmp_path / "stats.safetensors"), "--input_ids", ids,
                           "--device", "cuda:0", "--compute_dtype", "bfloat16", "--samples_output", smp,
                           "--n_sample_tokens", "128", "--log_level", "ERROR"]) == 0
    base = ["--model_id", str(src), "--output_format", "mxfp4", "--device", "cuda:0", "--log_level", "ERROR"]
    near, gptq = tmp_path / "near", tmp_path / "gptq"
    assert main(base + ["--output_dir", str(near)]) == 0
    assert main(base + ["--output_dir", str(gptq), "--mxfp4_rounding", "gptq", "--act_samples", smp]) == 0
    assert verify.main(["--model_id", str(src), "--quantized_dir", str(gptq), "--device", "cuda:0",
                        "--log_level", "CRITICAL"]) == 0
    qcfg = json.loads((gptq / "config.json").read_text())["quantization_config"]
    assert qcfg["rounding"] == "gptq" and qcfg["damp"] == 0.01 and qcfg["modules_to_not_convert"] == []
    assert json.loads((near / "config.json").read_text())["quantization_config"]["rounding"] == "nearest"

    a, b, samples = load_file(str(near / "model.safetensors")), load_file(str(gptq / "model.safetensors")), load_file(smp)
    assert sorted(a) == sorted(b)
    for name in a:                                          # lm_head and every other tensor without samples
        if not mc.BLOCK_LINEAR.match(name.replace("_scale", "")):
            assert torch.equal(a[name].view(torch.uint8), b[name].view(torch.uint8)), name
    loader = SafetensorsLoader(str(src), logger_level="WARNING")
    index = loader.tensor_index()
    keys = sample_keys(index, [i for i in index if mc.BLOCK_LINEAR.match(i.name)], "llama")
    loader.close()
    assert sorted(keys) == sorted(n for n in fx.state if mc.BLOCK_LINEAR.match(n))
    total = {"near": 0.0, "gptq": 0.0}
    for name, key in keys.items():
        W, X = fx.state[name].double().numpy(), samples[key].to(fx.state[name].dtype).double().numpy()
        for tag, d in (("near", a), ("gptq", b)):
            E = (ref.dequantize(d[name].numpy(), d[f"{name}_scale"].numpy()) - W) @ X.T
            total[tag] += float((E * E).sum())
    print(f"output error on the samples, grouped linears: nearest {total['near']:.6g}  gptq {total['gptq']:.6g}  "
          f"ratio {total['gptq'] / total['near']:.4f}")
    assert total["gptq"] < total["near"]
