"""--output_format mxfp4 --mxfp4_act_scales end to end on the llama fixture: main writes the
directory, verify returns 0 on it, 1 after one element of a folded norm weight is changed and 1 after one
scale byte is set to 255; the NumPy reader of tests/mxfp4_ref.py rebuilds every linear equal to evaluation's
dequantized weights; the fold is an equivalence of the whole model (model_cases.unquantized_fold within
model_cases.fold_bound, the MXFP4 error left out by forming the linears from the source in float64); and
every linear's bytes are quantize_mxfp4 of the source row-folded and scaled as the sidecar says."""
import json

import pytest
import torch
from safetensors.torch import load_file, save_file

import model_cases as mc
import mxfp4_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]


def test_directory_folds_and_verifies(tmp_path):
    from awq_quantizer import _hip, verify
    from awq_quantizer.evaluation import DeviceDequant, QuantizedCheckpoint
    from awq_quantizer.main import main
    from awq_quantizer.model_loading.safetensors_loader import SafetensorsLoader
    from awq_quantizer.quantization.awq import AWQQuantizer
    fx, src, out = mc.fixture("llama"), tmp_path / "src", tmp_path / "out"
    src.mkdir()
    save_file(dict(fx.state), str(src / "model.safetensors"), metadata={"format": "pt"})
    (src / "config.json").write_text(json.dumps(fx.config))
    assert main(["--model_id", str(src), "--output_dir", str(out), "--output_format", "mxfp4", "--mxfp4_scale", "mse",
                 "--mxfp4_act_scales", "--act_stats", fx.stats_path, "--device", "cuda:0", "--log_level", "ERROR"]) == 0

    written = load_file(str(out / "model.safetensors"))
    scales = load_file(str(out / "awq_scales.safetensors"))
    qcfg = json.loads((out / "config.json").read_text())["quantization_config"]
    assert (qcfg["quant_method"], qcfg["scale_rule"], qcfg["input_scales"]) == ("mxfp4", "mse", "awq")
    linears = sorted(n for n in fx.state if mc.BLOCK_LINEAR.match(n))
    assert sorted(n[: -len("_scale")] for n in written if n.endswith(".weight_scale")) == linears
    assert {k.rpartition(".")[0] for k in scales} == set(linears)
    rest = {n: t for n, t in written.items() if n in fx.state and n not in linears}
    changed = {n for n, t in rest.items() if not torch.equal(t, fx.state[n])}
    assert changed == {n for n in rest if "layernorm" in n}            # llama: no biases; every norm folded
    assert any(not torch.equal(s, torch.ones_like(s)) for s in scales.values())

    # the fold is an equivalence of the whole model
    e = fx.e(mc.unquantized_fold(fx, scales, rest))
    print(f"mxfp4 act fold llama: e {e:.3e}, bound {mc.fold_bound(fx, torch.bfloat16):.3e}")
    assert e <= mc.fold_bound(fx, torch.bfloat16)

    # every linear: the bytes of quantize_mxfp4 in the domain the sidecar records, read back by both readers
    q = AWQQuantizer(bits=4, group_size=128, device="cuda:0", logger_level="ERROR")
    loader = SafetensorsLoader(str(src), logger_level="WARNING")
    ckpt = QuantizedCheckpoint(loader, str(out), DeviceDequant("cuda:0"))
    index = {i.name: i for i in loader.tensor_index()}
    for name in linears:
        w = fx.state[name].cuda()
        if name + ".row_scale" in scales:
            w = _hip.fold_rows(w, scales[name + ".row_scale"].cuda())
        two = q.quantize_mxfp4(_hip.apply_input_scale(w, scales[name + ".input_scale"].cuda()), "mse")
        assert torch.equal(written[name], two["codes"].cpu()) and torch.equal(written[f"{name}_scale"], two["scales"].cpu())
        rebuilt = torch.from_numpy(ref.dequantize(written[name].numpy(), written[f"{name}_scale"].numpy())).float()
        got = ckpt.read(index[name]).cpu()
        assert torch.equal(got.view(torch.int32), rebuilt.view(torch.int32)), name
    ckpt.close()
    loader.close()

    argv = ["--model_id", str(src), "--quantized_dir", str(out), "--device", "cuda:0", "--log_level", "CRITICAL"]
    assert verify.main(argv) == 0
    report = json.loads((out / "quantization_error.json").read_text())
    assert sorted(report["tensors"]) == linears and report["fold_audited"] and report["totals"]["nonfinite"] == 0
    assert all(t["input_scaled"] for t in report["tensors"].values())
    norm, byte = sorted(changed)[0], f"{linears[0]}_scale"
    for key, at, blamed in ((norm, (3,), norm), (byte, (1, 0), linears[0])):   # a folded norm element; a scale byte
        bad = dict(written)
        bad[key] = written[key].clone()
        bad[key][at] = 255 if key == byte else bad[key][at] * 2 + 1
        save_file(bad, str(out / "model.safetensors"), metadata={"format": "pt"})
        assert verify.main(argv) == 1
        assert list(json.loads((out / "quantization_error.json").read_text())["problems"]) == [blamed]
