"""--output_format mxfp4 end to end on the llama fixture: main writes the directory, an
independent NumPy reader (tests/mxfp4_ref.py, from the format's definition) rebuilds every linear, the
result equals evaluation's dequantized weights bit for bit, verify returns 0 on the directory and 1 after
one scale byte of one tensor is set to 255."""
import json

import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

import model_cases as mc
import mxfp4_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]


def test_directory_reads_back_and_verifies(tmp_path):
    from awq_quantizer import verify
    from awq_quantizer.evaluation import DeviceDequant, QuantizedCheckpoint
    from awq_quantizer.main import main
    from awq_quantizer.model_loading.safetensors_loader import SafetensorsLoader
    fx, src, out = mc.fixture("llama"), tmp_path / "src", tmp_path / "out"
    src.mkdir()
    save_file(dict(fx.state), str(src / "model.safetensors"), metadata={"format": "pt"})
    (src / "config.json").write_text(json.dumps(fx.config))
    assert main(["--model_id", str(src), "--output_dir", str(out), "--output_format", "mxfp4", "--mxfp4_scale", "ceil",
                 "--device", "cuda:0", "--log_level", "ERROR"]) == 0

    written = load_file(str(out / "model.safetensors"))
    qcfg = json.loads((out / "config.json").read_text())["quantization_config"]
    assert (qcfg["quant_method"], qcfg["block_size"], qcfg["scale_rule"], qcfg["modules_to_not_convert"]) == \
        ("mxfp4", 32, "ceil", [])
    linears = sorted(n for n in fx.state if mc.BLOCK_LINEAR.match(n))
    assert sorted(n[: -len("_scale")] for n in written if n.endswith(".weight_scale")) == linears
    for name, t in fx.state.items():
        if name not in linears:
            assert torch.equal(written[name].view(torch.int16), t.view(torch.int16)), name

    loader = SafetensorsLoader(str(src), logger_level="WARNING")
    ckpt = QuantizedCheckpoint(loader, str(out), DeviceDequant("cuda:0"))
    assert ckpt.quantized_names() == linears
    index = {i.name: i for i in loader.tensor_index()}
    for name in linears:
        codes, scales = written[name].numpy(), written[f"{name}_scale"].numpy()
        assert codes.shape == (fx.state[name].shape[0], fx.state[name].shape[1] // 2)
        want_c, want_s, _ = ref.quantize(fx.state[name].double().numpy(), "ceil")
        assert np.array_equal(scales, want_s) and ((ref.nibbles(codes) == ref.nibbles(want_c)) |
                                                   (((ref.nibbles(codes) | ref.nibbles(want_c)) & 7) == 0)).all()
        rebuilt = torch.from_numpy(ref.dequantize(codes, scales)).float()
        got = ckpt.read(index[name]).cpu()
        assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), rebuilt.view(torch.int32)), name
    ckpt.close()
    loader.close()

    argv = ["--model_id", str(src), "--quantized_dir", str(out), "--device", "cuda:0", "--log_level", "CRITICAL"]
    assert verify.main(argv) == 0
    report = json.loads((out / "quantization_error.json").read_text())
    assert sorted(report["tensors"]) == linears and report["layout"] == "mxfp4" and report["totals"]["nonfinite"] == 0
    written[f"{linears[0]}_scale"][1, 0] = 255
    save_file(written, str(out / "model.safetensors"), metadata={"format": "pt"})
    assert verify.main(argv) == 1
    report = json.loads((out / "quantization_error.json").read_text())
    assert list(report["problems"]) == [linears[0]] and report["tensors"][linears[0]]["nonfinite"] == 32
