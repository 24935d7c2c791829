"""evaluate --mxfp4_activations on the llama fixture: main writes an MXFP4 directory, the CLI
evaluates it with the decoder linears in MXFP4 on both sides, and the per-token NLL of that run equals the same
forward with the ops' linear replaced by fake-quantize (dequantize_mxfp4(quantize_mxfp4(x))) + F.linear.

Tolerance: D = max |nll_q(torch forward, bf16) - nll_q(torch forward, fp32)| over the scored positions, both
with the fake-quantize linear; measured on an MI355X: D = 8.654e-03 (MEASURED_D; the kernel's own distance to
the fake-quantize fp32 forward was 0); asserted bound 2 D.  Without the flag nothing of the new path is
constructed and the result carries no new key."""
import json

import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import save_file

import model_cases as mc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]
MEASURED_D = 8.654e-03


def fake_quantize_linear(self, x, w, b=None):
    xq = self.q.dequantize_mxfp4(self.q.quantize_mxfp4(x, "floor"), x.dtype)
    return F.linear(xq, w.to(x.dtype), b)


def test_evaluate_with_mxfp4_activations(tmp_path, monkeypatch, capsys):
    import awq_quantizer.evaluation as ev
    from awq_quantizer import evaluate
    from awq_quantizer.main import main
    fx, src, out = mc.fixture("llama"), tmp_path / "src", tmp_path / "out"
    src.mkdir()
    save_file(dict(fx.state), str(src / "model.safetensors"), metadata={"format": "pt"})
    (src / "config.json").write_text(json.dumps(fx.config))
    save_file({"input_ids": fx.input_ids}, str(tmp_path / "ids.safetensors"))
    assert main(["--model_id", str(src), "--output_dir", str(out), "--output_format", "mxfp4", "--mxfp4_scale", "mse",
                 "--device", "cuda:0", "--log_level", "ERROR"]) == 0

    argv = ["--model_id", str(src), "--quantized_dir", str(out), "--input_ids", str(tmp_path / "ids.safetensors"),
            "--device", "cuda:0", "--compute_dtype", "float32", "--log_level", "ERROR"]
    assert evaluate.main(argv + ["--mxfp4_activations"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (line["activations"], line["head"], line["nonfinite_rows"]) == ("mxfp4", "dense", 0)
    assert all(torch.isfinite(torch.tensor(line[k])) for k in ("ppl_q", "ppl_ratio", "kl_mean", "kl_max"))

    def run(dtype, **kw):
        per = {}
        r = ev.evaluate_model(str(src), fx.input_ids, quantized_dir=str(out), compute_dtype=dtype, device="cuda:0",
                              per_token=per, **kw)
        return r, per["nll_q"].double()[per["targets"] >= 0]
    r_kernel, nll_kernel = run("float32", mxfp4_activations=True)
    assert json.dumps(r_kernel) == json.dumps(line)
    with monkeypatch.context() as m:
        m.setattr(ev.Mxfp4LinearOps, "linear", fake_quantize_linear)
        r32, nll32 = run("float32", mxfp4_activations=True)
        _, nll16 = run("bfloat16", mxfp4_activations=True)
    D = float((nll16 - nll32).abs().max())
    E = float((nll_kernel - nll32).abs().max())
    with capsys.disabled():
        print(f"W4A4 llama: ppl_q {r_kernel['ppl_q']:.5f} kl_mean {r_kernel['kl_mean']:.5e} (fake-quantize fp32: ppl_q "
              f"{r32['ppl_q']:.5f}); D = {D:.3e}, kernel vs fake-quantize E = {E:.3e} (bound {2 * MEASURED_D:.3e})")
    assert E <= 2 * MEASURED_D

    with monkeypatch.context() as m:        # without the flag: today's path, nothing of the new one is built
        m.setattr(ev, "Mxfp4LinearOps", lambda *a, **k: pytest.fail("Mxfp4LinearOps was built"))
        r_plain, nll_plain = run("float32")
    assert "activations" not in r_plain and "head" not in r_plain
    with capsys.disabled():
        print(f"W4A16 llama: ppl_q {r_plain['ppl_q']:.5f} kl_mean {r_plain['kl_mean']:.5e}")
    assert not torch.equal(nll_plain, nll_kernel)
    assert evaluate.main(argv) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == r_plain
