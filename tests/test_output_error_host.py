"""CPU-only tests of the output-space error's host layer (include/awq_hip.h awq_output_error,
DESIGN.md §5.13): the two C-ABI symbols are exported and bound, awq_output_error refuses what the
header says before any pointer is looked at, the workspace formula, the calibration pass's sample
rows, the new flag rules of main / calibrate / verify, and a numpy restatement of the kernel's
hi / lo bf16 split."""
import ctypes

import numpy as np
import pytest
import torch

BF16, F16, F32, F64, I32 = 0, 1, 2, 3, 4   # include/awq_hip.h AWQ_DTYPE_*
OK, EINVAL, EUNSUPPORTED = 0, 1, 2


def _lib():
    from awq_quantizer import _hip
    return _hip.load_library()


def _call(lib, *, w=0, dtype=BF16, N=4, K=256, gs=128, bits=4, sym=0, qweight=0, qzeros=0, scales=0, col=0, x=0, T=8,
          stride=None, work=0, err_sq=0, ref_sq=0, err=0):
    """awq_output_error with NULL device pointers: every refusal comes first."""
    P = ctypes.c_void_p
    return lib.awq_output_error(P(w), dtype, N, K, gs, bits, sym, P(qweight), P(qzeros), P(scales), P(col), P(x), T,
                                K if stride is None else stride, P(work), P(err_sq), P(ref_sq), P(err), None)


def test_symbols_exported_and_bound():
    from awq_quantizer import _hip
    lib = _lib()
    for name in ("awq_output_error", "awq_output_error_work_bytes"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert lib.awq_output_error_work_bytes.restype is ctypes.c_int64
    assert len(_hip.SIGNATURES["awq_output_error"][1]) == 19
    assert lib.awq_abi_version() == 17          # additive symbols: the ABI number stays
    assert callable(_hip.output_error)


def test_work_bytes():
    """fp32 [2 (E, R)][ceil(T / 128)][N]"""
    lib = _lib()
    assert lib.awq_output_error_work_bytes(4096, 512) == 2 * 4 * 4096 * 4
    assert lib.awq_output_error_work_bytes(130, 129) == 2 * 2 * 130 * 4
    assert lib.awq_output_error_work_bytes(1, 1) == 8
    assert lib.awq_output_error_work_bytes(7, 128) == 56 and lib.awq_output_error_work_bytes(7, 129) == 112
    assert lib.awq_output_error_work_bytes(0, 5) == 0 and lib.awq_output_error_work_bytes(5, 0) == 0
    assert lib.awq_output_error_work_bytes(-1, 5) == 0
    assert lib.awq_output_error_work_bytes(1 << 40, 1 << 30) == 0      # N T above 2^60


REFUSALS = [
    (dict(dtype=F64), EUNSUPPORTED), (dict(dtype=I32), EINVAL), (dict(dtype=-1), EINVAL),
    (dict(bits=3), EINVAL), (dict(bits=16), EINVAL),
    (dict(gs=0), EINVAL), (dict(gs=-8), EINVAL), (dict(gs=4), EUNSUPPORTED), (dict(gs=96, K=192), EUNSUPPORTED),
    (dict(gs=1024, K=1024), EUNSUPPORTED),
    (dict(K=200), EUNSUPPORTED),                                   # K % group_size
    (dict(stride=255), EINVAL), (dict(stride=0), EINVAL),
    (dict(N=1 << 40, K=1 << 30, gs=128), EUNSUPPORTED), (dict(N=1 << 40, T=1 << 30), EUNSUPPORTED),
    (dict(N=-1), EINVAL), (dict(K=-256), EINVAL), (dict(T=-1), EINVAL),
    (dict(), EINVAL),                                              # a valid shape: the NULL pointers
    (dict(w=0x1001, x=0x2000, qweight=0x3000, qzeros=0x4000, scales=0x5000, work=0x6000, err_sq=0x7000), EINVAL),
]


def test_refusals_come_before_any_pointer_is_looked_at():
    from awq_quantizer import _hip
    for kw, code in REFUSALS:
        assert _call(_lib(), **kw) == code, kw
        assert _hip.last_error() != "", kw


def test_empty_shapes_return_before_the_pointers():
    for kw in (dict(N=0), dict(K=0), dict(T=0)):
        assert _call(_lib(), **kw) == OK, kw


def test_sample_rows():
    from awq_quantizer.calibration import sample_rows
    assert sample_rows(10, 4) == [0, 2, 5, 7]
    assert sample_rows(1024, 512) == list(range(0, 1024, 2))
    assert sample_rows(7, 7) == list(range(7)) and sample_rows(3, 8) == [0, 1, 2]
    assert sample_rows(5, 0) == [] and sample_rows(0, 4) == [] and sample_rows(5, -1) == []
    for total, n in ((1000, 512), (513, 512), (97, 13)):
        rows = sample_rows(total, n)
        assert len(rows) == n and rows == sorted(set(rows)) and rows[0] == 0 and rows[-1] < total
        assert all(r == j * total // n for j, r in enumerate(rows))


def test_run_decoder_signature_keeps_nothing_by_default():
    import inspect
    from awq_quantizer.calibration import calibrate_model, run_decoder
    for fn in (run_decoder, calibrate_model):
        p = inspect.signature(fn).parameters
        assert p["n_sample_tokens"].default == 0 and p["samples_out"].default is None


def test_load_act_samples_maps_weights_to_their_groups_tensor(tmp_path):
    from awq_quantizer.calibration import load_act_samples, save_act_samples
    flat = {"model.layers.0.attn_in.samples": torch.arange(6.0).reshape(2, 3).to(torch.bfloat16),
            "model.layers.0.mlp_out.samples": torch.ones(2, 5), "model.layers.1.attn_out.samples": torch.zeros(1, 4)}
    path = str(tmp_path / "sub" / "samples.safetensors")
    save_act_samples(flat, path)
    got = load_act_samples(path)
    assert set(got) == {f"model.layers.0.self_attn.{m}_proj.weight" for m in "qkv"} | {
        "model.layers.0.mlp.down_proj.weight", "model.layers.1.self_attn.o_proj.weight"}
    assert torch.equal(got["model.layers.0.self_attn.k_proj.weight"], flat["model.layers.0.attn_in.samples"])
    assert got["model.layers.0.self_attn.k_proj.weight"].dtype == torch.bfloat16
    assert torch.equal(got["model.layers.0.mlp.down_proj.weight"], torch.ones(2, 5))


BASE = ["--model_id", "m", "--output_dir", "o"]
FOLD = ["--scale_method", "awq", "--output_format", "autoawq", "--fold_scales"]


def test_search_loss_flag_rules():
    from awq_quantizer.options import check_flags, parse_args
    a = parse_args(BASE)
    assert (a.search_loss, a.act_samples, a.n_sample_tokens) == ("diag", None, 512)
    ok = [FOLD + ["--act_stats", "s", "--search_loss", "output", "--act_samples", "x"],
          FOLD + ["--calib_ids", "ids", "--search_loss", "output"],
          FOLD + ["--calib_ids", "ids", "--search_loss", "output", "--n_sample_tokens", "64"],
          FOLD + ["--act_stats", "s"], FOLD + ["--act_stats", "s", "--search_loss", "diag"]]
    for argv in ok:
        assert check_flags(parse_args(BASE + argv)) is None, argv
    bad = {"needs --fold_scales": ["--scale_method", "awq", "--act_stats", "s", "--search_loss", "output",
                                   "--act_samples", "x"],
           "needs token samples": FOLD + ["--act_stats", "s", "--search_loss", "output"],
           "one of them": FOLD + ["--calib_ids", "ids", "--search_loss", "output", "--act_samples", "x"],
           "--n_sample_tokens must be positive": FOLD + ["--calib_ids", "ids", "--search_loss", "output",
                                                         "--n_sample_tokens", "0"],
           "is read by --search_loss output": FOLD + ["--act_stats", "s", "--act_samples", "x"]}
    for want, argv in bad.items():
        err = check_flags(parse_args(BASE + argv))
        assert err is not None and want in err, (want, err)
    with pytest.raises(SystemExit):
        parse_args(BASE + ["--search_loss", "mse"])


def test_missing_samples_file_is_an_error_before_the_model_is_read(tmp_path):
    from awq_quantizer import main
    argv = ["--model_id", str(tmp_path / "no_such_model"), "--output_dir", str(tmp_path / "o"), "--log_level",
            "CRITICAL"] + FOLD + ["--act_stats", "s", "--search_loss", "output", "--act_samples", str(tmp_path / "none")]
    assert main.main(argv) == 1


def test_verify_and_calibrate_argument_parsing():
    from awq_quantizer import calibrate, verify
    a = verify.parse_args(["--model_id", "s", "--quantized_dir", "o"])
    assert a.act_samples is None
    a = verify.parse_args(["--model_id", "s", "--quantized_dir", "o", "--act_samples", "x.safetensors"])
    assert a.act_samples == "x.safetensors"
    c = calibrate.build_parser().parse_args(["--model_id", "m", "--output", "s", "--input_ids", "i"])
    assert (c.samples_output, c.n_sample_tokens) == (None, 512)
    c = calibrate.build_parser().parse_args(["--model_id", "m", "--output", "s", "--input_ids", "i", "--samples_output",
                                             "x", "--n_sample_tokens", "64"])
    assert (c.samples_output, c.n_sample_tokens) == ("x", 64)


def test_verify_passes_samples_on_and_adds_the_output_figures(tmp_path):
    """Stubbed error function: a linear with samples is measured with samples=, its entry and the
    totals gain the output figures; without --act_samples the call and the report are today's."""
    import json
    from safetensors.torch import save_file
    from awq_quantizer import verify
    from awq_quantizer.calibration import save_act_samples
    from awq_quantizer.main import save_model_in_chunks
    from awq_quantizer.quantization.awq import error_report, output_report
    src = tmp_path / "src"
    src.mkdir()
    names = ["model.layers.0.self_attn.o_proj.weight", "other.weight"]
    save_file({n: torch.zeros(4, 256, dtype=torch.bfloat16) for n in names}, str(src / "model.safetensors"))
    res = {n: {"scales": torch.ones((4, 2), dtype=torch.float16), "bits": torch.tensor(4, dtype=torch.int32),
               "group_size": torch.tensor(128, dtype=torch.int32), "symmetric": torch.tensor(False),
               "qweight": torch.zeros((4, 32), dtype=torch.int32), "qzeros": torch.zeros((4, 1), dtype=torch.int32),
               "shape": torch.tensor([4, 256], dtype=torch.int64)} for n in names}
    out = tmp_path / "out"
    save_model_in_chunks(res, str(out), chunk_size=10)
    smp = tmp_path / "samples.safetensors"
    save_act_samples({"model.layers.0.attn_out.samples": torch.ones(6, 256, dtype=torch.bfloat16)}, str(smp))
    calls = []

    def stub(tensor, result, **kw):
        calls.append(sorted(kw))
        e = error_report(tensor.numel(), [1.0, 1.0, 4.0, 1.0, 0.0])
        if "samples" in kw:
            e.update(output_report(2.0, 200.0, kw["samples"].shape[0]))
        return e

    base = ["--model_id", str(src), "--quantized_dir", str(out), "--log_level", "ERROR"]
    assert verify.verify(verify.parse_args(base), error_fn=stub) == 0
    plain = json.load(open(out / "quantization_error.json"))
    assert calls == [[], []]
    assert not any(k.startswith("output_") for e in [plain["totals"], *plain["tensors"].values()] for k in e)
    calls.clear()
    assert verify.verify(verify.parse_args(base + ["--act_samples", str(smp), "--report", str(tmp_path / "r.json")]),
                         error_fn=stub) == 0
    assert sorted(calls) == [[], ["samples"]]
    rep = json.load(open(tmp_path / "r.json"))
    e = rep["tensors"][names[0]]
    assert (e["output_sum_sq"], e["output_ref_sq"], e["output_tokens"], e["output_snr_db"]) == (2.0, 200.0, 6, 20.0)
    assert "output_sum_sq" not in rep["tensors"]["other.weight"]
    t = rep["totals"]
    assert (t["output_sum_sq"], t["output_ref_sq"], t["output_tensors"], t["output_snr_db"]) == (2.0, 200.0, 1, 20.0)
    assert verify.worst_by_output(rep["tensors"], 5) == [names[0]]
    assert verify.verify(verify.parse_args(base + ["--act_samples", str(tmp_path / "missing")]), error_fn=stub) == 1


# ---------------------------------------------------------------- the hi / lo split, restated in numpy
def rn_bf16(a: np.ndarray) -> np.ndarray:
    """round-to-nearest-even of float32 to bf16, returned as float32 (finite inputs)"""
    u = a.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split(d: np.ndarray):
    hi = rn_bf16(d)
    return hi, rn_bf16((d - hi).astype(np.float32))


def test_split_is_exact_on_the_exact_data_construction():
    """d = (q - z) / c - m 2^-8 with |q - z| <= 31, c in {1/2, 1, 2}, m in [0, 255]: hi + lo == d"""
    rng = np.random.default_rng(0)
    diff = rng.integers(-31, 32, size=1 << 16).astype(np.float32)
    c = (2.0 ** rng.integers(-1, 2, size=diff.size)).astype(np.float32)
    d = (diff / c - rng.integers(0, 256, size=diff.size).astype(np.float32) / 256).astype(np.float32)
    hi, lo = split(d)
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), d.astype(np.float64))
    assert (lo != 0).mean() > 0.7           # dropping or misplacing the low half is visible


def test_split_error_on_random_data_stays_under_the_bound():
    for K in (256, 4096):
        _split_error(K)


def _split_error(K):
    """Per element the worst case is |hi + lo - d| <= 2^-17 |d| (bf16 keeps 8 significant bits:
    |d - hi| <= 2^-8 2^e, so lo's exponent is at most e - 9 and its rounding errs by at most
    2^(e - 17)) — eps_K's first term; over a row of random data the split product stays under
    2^-18 A, and with an fp32 matmul on top the total stays far inside eps_K = 2^-17 + K 2^-22."""
    rng = np.random.default_rng(K)
    d = (rng.standard_normal((16, K)) * 0.01).astype(np.float32)
    x = rn_bf16(rng.standard_normal((24, K)).astype(np.float32))
    hi, lo = split(d)
    s = hi.astype(np.float64) + lo.astype(np.float64)
    assert np.all(np.abs(s - d) <= 2.0 ** -17 * np.abs(d))
    A = np.abs(d).astype(np.float64) @ np.abs(x).astype(np.float64).T
    exact = d.astype(np.float64) @ x.astype(np.float64).T
    assert np.all(np.abs(s @ x.astype(np.float64).T - exact) <= 2.0 ** -18 * A)
    got = (hi @ x.T + lo @ x.T).astype(np.float64)                 # fp32 accumulation, numpy's order
    rel = float((np.abs(got - exact) / A).max())
    print(f"split + fp32 matmul, K = {K}: max error {rel:.2e} A (eps_K = {2.0 ** -17 + K * 2.0 ** -22:.2e})")
    assert rel <= 2.0 ** -17 + K * 2.0 ** -22
