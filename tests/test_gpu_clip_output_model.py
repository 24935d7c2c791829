"""The token-sample clip loss from the calibration pass to a written checkpoint, on the committed
tests/golden/model_llama fixture: main --calib_ids --fold_scales --act_clip
--clip_loss output, the checkpoint read back by tests/checkpoint_reader.py + tests/model_forward.py
as test_gpu_model_forward.py does, beside the --clip_loss diag run.

Measured on an MI355X (llama bf16, group size 32, 128 calibration tokens, all kept as samples):
  e_textbook-RTN 6.181e-03; --clip_loss diag e / e_textbook 0.714, --clip_loss output 0.678
  (e_output / e_diag 0.950); summed group losses after / before clipping: 0.8789 (diag run, diagonal
  loss), 0.8623 (output run, output loss).
No ordering between the two clip losses is asserted: one 2-block model and 128 tokens do not carry
one.  Asserted: the run writes a loadable checkpoint whose bytes differ from the
diagonal clip's, every layer group's logged output loss does not grow under clipping, and the
logit error stays inside THETA * e_textbook like every other written checkpoint's.

part_checkpoint is run by tests/test_gpu_clip_output.py::test_clip_output (one test id for the
feature's GPU checks); this file holds no test id of its own.
"""
import json
import os
import re

import torch
from safetensors.torch import save_file

import model_cases as mc
from checkpoint_reader import read_checkpoint
from test_gpu_calibrate import calib_ids

TOKENS = 128           # calib_ids: 4 sequences of 32 tokens, all kept
CLIP_LINE = re.compile(r"(\S+\.(?:attn_in|attn_out|mlp_in|mlp_out)): clip loss (\w+), (\S+) -> (\S+)")


def part_checkpoint(tmp_path):
    from awq_quantizer import _hip
    from awq_quantizer.main import main
    _hip.require_device(torch.device("cuda", 0))
    fx = mc.fixture("llama")
    model = tmp_path / "model"
    model.mkdir()
    save_file(dict(fx.state), str(model / "model.safetensors"), metadata={"format": "pt"})
    with open(model / "config.json", "w") as f:
        json.dump(fx.config, f)
    ids = str(tmp_path / "ids.safetensors")
    save_file({"input_ids": calib_ids("llama")}, ids)
    common = ["--model_id", str(model), "--group_size", "32", "--device", "cuda:0", "--output_format", "autoawq",
              "--scale_method", "awq", "--fold_scales", "--calib_ids", ids, "--act_clip", "--n_sample_tokens", str(TOKENS)]
    outs = {k: str(tmp_path / k) for k in ("diag", "output", "default")}
    logs = {k: str(tmp_path / f"{k}.log") for k in outs}
    assert main(common + ["--output_dir", outs["diag"], "--clip_loss", "diag", "--log_file", logs["diag"]]) == 0
    assert main(common + ["--output_dir", outs["output"], "--clip_loss", "output", "--log_file", logs["output"]]) == 0
    assert main(common + ["--output_dir", outs["default"], "--log_file", logs["default"]]) == 0

    def data(k, f="model.safetensors"):
        return open(os.path.join(outs[k], f), "rb").read()

    assert data("default") == data("diag")                    # no flag: the diagonal clip
    assert data("output") != data("diag")
    assert data("output", "awq_scales.safetensors") == data("diag", "awq_scales.safetensors")   # the same scale search

    lines = {k: CLIP_LINE.findall(open(logs[k]).read()) for k in ("diag", "output")}
    for k in ("diag", "output"):
        assert len(lines[k]) == 4 * fx.layers, lines[k]
        for group, how, before, after in lines[k]:
            assert how == k and float(after) <= float(before), (group, how, before, after)
    log = open(logs["output"]).read()
    assert len(re.findall(r"awq clip \S+: clipped .* output loss ", log)) == len(fx.quantized_names("autoawq"))
    ratio = {k: sum(float(a) for *_, a in lines[k]) / sum(float(b) for _, _, b, _ in lines[k]) for k in lines}

    e = {k: fx.e(read_checkpoint(outs[k])[0]) for k in ("diag", "output")}
    et = mc.e_textbook("llama", "autoawq", 32)
    print(f"clip loss llama bf16 gs32: e_textbook {et:.3e}  diag clip e/e_textbook {e['diag'] / et:.3f}  output clip "
          f"e/e_textbook {e['output'] / et:.3f}  e_output/e_diag {e['output'] / e['diag']:.3f}; summed group losses "
          f"after / before: diag (diagonal loss) {ratio['diag']:.4f}, output (output loss) {ratio['output']:.4f}")
    assert e["output"] < mc.THETA * et
