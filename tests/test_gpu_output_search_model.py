"""The output-space loss from the calibration pass to a written checkpoint, on the committed
tests/golden/model_llama fixture: calibrate --samples_output, main --calib_ids
--fold_scales --search_loss output, verify --act_samples, and the checkpoint read back by
tests/checkpoint_reader.py + tests/model_forward.py as test_gpu_model_forward.py does.

Measured on an MI355X (llama bf16, group size 32, 128 calibration tokens, all kept as samples):
  samples vs statistics, max relative difference of a column's mean square: fp32 5.8e-08, bf16 5.7e-08
  e_textbook-RTN 6.181e-03, written RTN checkpoint e_rtn 6.107e-03;
  --fold_scales with the diagonal loss: e / e_textbook 0.735;
  with --search_loss output: e / e_textbook 0.738 (e_output / e_rtn 0.747, e_output / e_diag 1.003);
  verify --act_samples: model output SNR 27.49 dB.
  Winners (output / diagonal, of 20): attn_in 8 / 8 and mlp_in 8 / 8 in both blocks; attn_out 5 / 5
  and 10 / 6; mlp_out 3 / 6 and 9 / 7; the winner's output loss over candidate 0's: 0.23 .. 0.87.
e_output <= e_rtn is asserted: the measured ratio (1 / 0.747 = 1.34) leaves more than the 1.2x
margin the project asks of such an assertion.  e_output <= e_diag is NOT asserted: on this 2-block
model and 128 tokens the two searches agree on four of eight groups and the checkpoints' logit
errors differ by 0.3 %, far below that margin; both are far inside THETA * e_textbook.
"""
import json
import os

import pytest
import torch
from safetensors.torch import load_file, save_file

import model_cases as mc
from checkpoint_reader import read_checkpoint
from test_gpu_calibrate import calib_ids

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]

DTYPES = {"fp32": "float32", "bf16": "bfloat16"}
GROUPS = {"attn_in": "self_attn.q_proj", "attn_out": "self_attn.o_proj", "mlp_in": "mlp.gate_proj",
          "mlp_out": "mlp.down_proj"}
TOKENS = 128           # calib_ids: 4 sequences of 32 tokens, all kept


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """The model directory, the ids file, and calibrate --samples_output run once per precision."""
    from awq_quantizer import _hip, calibrate
    _hip.require_device(torch.device("cuda", 0))
    fx = mc.fixture("llama")
    root = tmp_path_factory.mktemp("output_search")
    model = root / "model"
    model.mkdir()
    save_file(dict(fx.state), str(model / "model.safetensors"), metadata={"format": "pt"})
    with open(model / "config.json", "w") as f:
        json.dump(fx.config, f)
    ids = str(root / "ids.safetensors")
    save_file({"input_ids": calib_ids("llama")}, ids)
    done = {}

    def calibrated(prec):
        if prec not in done:
            stats, smp = str(root / f"stats_{prec}.safetensors"), str(root / f"samples_{prec}.safetensors")
            assert calibrate.main(["--model_id", str(model), "--output", stats, "--input_ids", ids, "--device", "cuda:0",
                                   "--compute_dtype", DTYPES[prec], "--samples_output", smp, "--n_sample_tokens",
                                   str(TOKENS), "--log_level", "ERROR"]) == 0
            done[prec] = (stats, smp)
        return done[prec]

    return {"fx": fx, "root": root, "model": str(model), "ids": ids, "calibrated": calibrated}


def test_samples(work):
    """n_sample_tokens = all tokens: each group's column mean of squares of the samples (float64) is
    the statistics file's x_sq — 1e-5 relative in fp32, the rounding of the dtype (2^-8) in bf16 —
    and the statistics file has exactly the keys it has without --samples_output; load_act_samples
    names every block linear."""
    from awq_quantizer.calibration import load_act_samples
    for prec in ("fp32", "bf16"):
        _samples_reproduce_the_statistics(work, prec)
    fx = work["fx"]
    by_weight = load_act_samples(work["calibrated"]("bf16")[1])
    assert set(by_weight) == set(fx.quantized_names("autoawq"))
    for name, t in by_weight.items():
        assert t.shape[1] == fx.names[name][1]


def _samples_reproduce_the_statistics(work, prec):
    fx = work["fx"]
    stats_path, smp_path = work["calibrated"](prec)
    stats, smp = load_file(stats_path), load_file(smp_path)
    assert set(stats) == set(fx.stats)
    assert set(smp) == {f"model.layers.{i}.{g}.samples" for i in range(fx.layers) for g in GROUPS}
    tol = {"fp32": 1e-5, "bf16": 2.0 ** -8}[prec]
    worst = 0.0
    for key, t in smp.items():
        block, group = key[: -len(".samples")].rsplit(".", 1)
        ref = stats[f"{block}.{GROUPS[group]}.weight.x_sq"].double()
        assert t.dtype == getattr(torch, DTYPES[prec]) and tuple(t.shape) == (TOKENS, ref.numel())
        got = (t.double() ** 2).mean(dim=0)
        assert bool(((got - ref).abs() <= tol * ref.abs()).all()), (prec, key)
        worst = max(worst, float(((got - ref).abs() / ref.abs()).max()))
    print(f"samples vs statistics {prec}: max relative difference {worst:.3e} (bound {tol:.3e})")


def test_checkpoint(work):
    """main --calib_ids --fold_scales --search_loss output: verify --act_samples accepts the
    checkpoint and reports the output figures of every linear; its float64 logits against the
    textbook RTN's, beside the diagonal search's."""
    from awq_quantizer import verify
    from awq_quantizer.main import main
    fx, root = work["fx"], work["root"]
    common = ["--model_id", work["model"], "--log_level", "ERROR", "--group_size", "32", "--device", "cuda:0",
              "--output_format", "autoawq"]
    awq = ["--scale_method", "awq", "--fold_scales", "--calib_ids", work["ids"]]
    outs = {k: str(root / k) for k in ("rtn", "diag", "output", "from_file")}
    assert main(common + ["--output_dir", outs["rtn"]]) == 0
    assert main(common + awq + ["--output_dir", outs["diag"]]) == 0
    assert main(common + awq + ["--output_dir", outs["output"], "--search_loss", "output", "--n_sample_tokens",
                                str(TOKENS)]) == 0
    stats_path, smp_path = work["calibrated"]("bf16")
    # the same run from the two files calibrate wrote: the same bytes
    assert main(common + ["--scale_method", "awq", "--fold_scales", "--act_stats", stats_path, "--search_loss",
                          "output", "--act_samples", smp_path, "--output_dir", outs["from_file"]]) == 0
    for f in ("model.safetensors", "awq_scales.safetensors"):
        assert open(os.path.join(outs["output"], f), "rb").read() == open(os.path.join(outs["from_file"], f), "rb").read()

    report = str(root / "report.json")
    assert verify.main(["--model_id", work["model"], "--quantized_dir", outs["output"], "--act_samples", smp_path,
                        "--report", report, "--log_level", "ERROR"]) == 0
    rep = json.load(open(report))
    assert set(rep["tensors"]) == set(fx.quantized_names("autoawq")) and rep["problems"] == {}
    for name, e in rep["tensors"].items():
        assert e["output_tokens"] == TOKENS and 0.0 < e["output_sum_sq"] < e["output_ref_sq"], name
        assert e["output_snr_db"] > 10.0, name
    t = rep["totals"]
    assert t["output_tensors"] == len(rep["tensors"])
    assert t["output_sum_sq"] == pytest.approx(sum(e["output_sum_sq"] for e in rep["tensors"].values()), rel=1e-12)
    # without the flag: today's report
    plain = str(root / "plain.json")
    assert verify.main(["--model_id", work["model"], "--quantized_dir", outs["output"], "--report", plain,
                        "--log_level", "ERROR"]) == 0
    plain_rep = json.load(open(plain))
    assert not any(k.startswith("output_") for e in [plain_rep["totals"], *plain_rep["tensors"].values()] for k in e)

    e = {k: fx.e(read_checkpoint(outs[k])[0]) for k in ("rtn", "diag", "output")}
    et = mc.e_textbook("llama", "autoawq", 32)
    print(f"output search llama bf16 gs32: e_textbook {et:.3e}  e_rtn {e['rtn']:.3e}  diag e/e_textbook "
          f"{e['diag'] / et:.3f}  output e/e_textbook {e['output'] / et:.3f}  e_output/e_rtn "
          f"{e['output'] / e['rtn']:.3f}  e_output/e_diag {e['output'] / e['diag']:.3f}  model output snr "
          f"{t['output_snr_db']:.2f} dB")
    assert e["output"] < mc.THETA * et
    assert e["output"] <= e["rtn"]          # module docstring: the measured ratio leaves the 1.2x margin


def test_group_winners(work):
    """quantize_block(loss="output") on the fixture's blocks: per layer group the chosen candidate's
    output loss is <= candidate 0's (s = 1 up to the normalisation), and the report names both winners."""
    from awq_quantizer.calibration import load_act_samples  # noqa: F401  (the file's layout is the API's)
    from awq_quantizer.main import load_act_stats
    from awq_quantizer.quantization import AWQQuantizer
    from awq_quantizer.quantization.block_plan import plan_blocks
    fx = work["fx"]
    stats_path, smp_path = work["calibrated"]("bf16")
    stats, smp = load_act_stats(stats_path), load_file(smp_path)
    q = AWQQuantizer(bits=4, group_size=32, symmetric=False, device="cuda:0", scale_method="awq", logger_level="ERROR")
    plan = plan_blocks({n: tuple(t.shape) for n, t in fx.state.items()}, "llama", 32)
    assert len(plan) == fx.layers
    for block in plan:
        samples = {g: smp[f"{block.prefix}.{g}.samples"] for g in block.groups}
        out = q.quantize_block({n: fx.state[n] for n in block.tensor_names()}, stats, block, loss="output",
                               samples=samples)
        plain = q.quantize_block({n: fx.state[n] for n in block.tensor_names()}, stats, block)
        for gname, g in out["groups"].items():
            assert g["folded"] and g["loss"] == "output", gname
            losses = g["losses"].cpu()
            assert float(losses[g["best"]]) <= float(losses[0]), (block.prefix, gname)
            assert g["best"] == int(torch.argmin(losses)) and "loss" not in plain["groups"][gname]
            print(f"{block.prefix}.{gname}: output winner {g['best']}  diagonal winner {g['diag_best']}  "
                  f"loss / loss[0] {float(losses[g['best']] / losses[0]):.4f}")
        # a group without samples falls back to the diagonal loss
        partial = q.quantize_block({n: fx.state[n] for n in block.tensor_names()}, stats, block, loss="output",
                                   samples={"attn_in": samples["attn_in"]})
        assert partial["groups"]["attn_in"].get("loss") == "output" and "loss" not in partial["groups"]["mlp_out"]
