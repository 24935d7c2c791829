"""Quantization-error report on the GPU (include/awq_hip.h awq_quant_error, AWQQuantizer.
quantization_error, awq_quantizer.verify), bit for bit against an expectation put together on
the CPU from independent pieces:
  * orc.dequantize — the golden-pinned reference dequantize — gives the fp32 dq;
  * level 1 (per group, fp32) is restated below in numpy float32: the 8-element chunk loops and
    the pairwise tree over 64 chunk slots;
  * orc.act_search_select gives the level-2 fp64 sums (the four-level order).
Group arrays are compared as int32 bit patterns, totals as float64 bit patterns."""
import json
import math

import numpy as np
import pytest
import torch

from oracle import awq_oracle as orc

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from awq_quantizer import _hip
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    return dev


_Q = {}


def quantizer(bits=4, gs=128, sym=False):
    from awq_quantizer.quantization import AWQQuantizer
    key = (bits, gs, sym)
    if key not in _Q:
        _Q[key] = AWQQuantizer(bits=bits, group_size=gs, symmetric=sym, device="cuda:0", logger_level="ERROR")
    return _Q[key]


# ---------------------------------------------------------------- the expectation (CPU)
def group_sum(v: np.ndarray, gs: int) -> np.ndarray:
    """float32 [R, K] (>= +0) -> the canonical fp32 sum of every group, float32 [R, G]."""
    R, K = v.shape
    G = -(-K // gs)
    k = np.arange(K)
    slots = np.zeros((R, G * 512), dtype=F32)          # every group padded to 64 chunk slots of 8 (+0)
    slots[:, (k // gs) * 512 + (k % gs)] = v
    slots = slots.reshape(R, G, 64, 8)
    acc = np.zeros((R, G, 64), dtype=F32)
    for j in range(8):                                 # chunk c = elements 8c .. 8c+7 in sequence from +0
        acc = (acc + slots[..., j]).astype(F32)
    while acc.shape[-1] > 1:                           # pairwise tree, adjacent pairs first
        acc = (acc[..., 0::2] + acc[..., 1::2]).astype(F32)
    return acc[..., 0]


def level1(w32: np.ndarray, dq: np.ndarray, gs: int):
    """w32, dq: float32 [R, K].  -> (sum_a, sum_e, sum_p, max_a) float32 [R, G], count int32 [R, G]."""
    R, K = w32.shape
    G = -(-K // gs)
    with np.errstate(all="ignore"):
        d = (w32 - dq).astype(F32)
        a, e, p = np.abs(d), (d * d).astype(F32), (w32 * w32).astype(F32)
    fin = np.isfinite(d) & np.isfinite(e) & np.isfinite(p)
    a, e, p = (np.where(fin, v, F32(0)).astype(F32) for v in (a, e, p))
    pad = G * gs - K
    gmax = np.pad(a, ((0, 0), (0, pad))).reshape(R, G, gs).max(axis=-1)
    bad = np.pad(~fin, ((0, 0), (0, pad))).reshape(R, G, gs).sum(axis=-1).astype(np.int32)
    return group_sum(a, gs), group_sum(e, gs), group_sum(p, gs), gmax, bad


def expect(x: torch.Tensor, ref: dict):
    """ref: a reference-format dict (tensor_q / scales / zero_points / group_size) on the CPU."""
    gs = int(ref["group_size"].item())
    rows = 1 if x.dim() <= 1 else x.shape[0]
    w32 = x.detach().cpu().float().reshape(rows, -1).numpy()
    dq = orc.dequantize(ref).reshape(rows, -1).numpy()
    sa, se, sp, gm, bad = level1(w32, dq, gs)
    part = torch.from_numpy(np.stack([sa.reshape(-1), se.reshape(-1), sp.reshape(-1)]))
    sums, _ = orc.act_search_select(part)
    return {"group_abs": sa, "group_sq": se, "group_w_sq": sp, "group_max": gm, "group_nonfinite": bad,
            "totals": np.array([*sums.tolist(), float(gm.max()), float(bad.sum(dtype=np.int64))], dtype=np.float64),
            "numel": x.numel()}


def check(got: dict, want: dict):
    for k in ("group_abs", "group_sq", "group_w_sq", "group_max"):
        g = got[k].cpu().numpy()
        assert g.dtype == F32 and g.shape == want[k].shape, k
        assert np.array_equal(g.view(np.int32), want[k].view(np.int32)), k
    assert got["group_nonfinite"].dtype == torch.int32
    assert np.array_equal(got["group_nonfinite"].cpu().numpy(), want["group_nonfinite"])
    tot = np.array([got["sum_abs"], got["sum_sq"], got["sum_w_sq"], got["max_abs_error"], float(got["nonfinite"])],
                   dtype=np.float64)
    assert np.array_equal(tot.view(np.int64), want["totals"].view(np.int64)), (tot, want["totals"])
    n, bad = want["numel"], int(want["totals"][4])
    assert (got["numel"], got["nonfinite"]) == (n, bad)
    assert all(type(got[k]) in (int, float) for k in ("numel", "nonfinite", "sum_abs", "sum_sq", "sum_w_sq",
                                                     "mean_abs_error", "mse", "max_abs_error", "snr_db"))
    if n == bad:
        assert math.isnan(got["mean_abs_error"]) and math.isnan(got["mse"])
    else:
        assert got["mean_abs_error"] == want["totals"][0] / (n - bad) and got["mse"] == want["totals"][1] / (n - bad)
    if want["totals"][1] == 0.0:
        assert got["snr_db"] == math.inf
    else:
        assert got["snr_db"] == 10.0 * math.log10(want["totals"][2] / want["totals"][1])


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    view = {torch.float32: torch.int32, torch.float64: torch.int64}.get(a.dtype, a.dtype)
    return a.dtype == b.dtype and torch.equal(a.view(view), b.view(view))


def weights(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 0.05).to(dtype)


def packed_of(ref: dict, shape) -> dict:
    """The packed dict of a reference-format result, packed on the CPU (orc.pack_rows)."""
    bits, sym = int(ref["bits"].item()), bool(ref["symmetric"].item())
    qmin = orc.qrange(bits, sym)[0]
    rows = 1 if len(shape) <= 1 else shape[0]
    return {"qweight": orc.pack_rows(ref["tensor_q"].reshape(rows, -1), bits, qmin),
            "qzeros": orc.pack_rows(ref["zero_points"], bits, qmin), "scales": ref["scales"], "bits": ref["bits"],
            "group_size": ref["group_size"], "symmetric": ref["symmetric"],
            "shape": torch.tensor(list(shape), dtype=torch.int64)}


def tie_to_reference_figure(x, ref, got):
    """The reference's own figure (its test_quantization.py:155-160).  torch's fp32 cascade sum over
    <= 2^20 elements errs by about 20 * 2^-24 = 1.2e-6 relative; the tolerance is 10 x that."""
    want = torch.abs(x.cpu() - orc.dequantize(ref)).mean().item()
    assert got["mean_abs_error"] == pytest.approx(want, rel=1e-5)


# ---------------------------------------------------------------- RTN results via quantize_packed
@pytest.mark.parametrize("shape", [(3, 256), (64, 1024), (17, 384), (1024,)])
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_rtn_results(dtype, bits, sym, shape):
    _dev()
    x = weights(shape, dtype, seed=bits + len(shape))
    q = quantizer(bits, 128, sym)
    got = q.quantization_error(x, q.quantize_packed(x), per_group=True)
    ref = orc.quantize(x, bits=bits, group_size=128, symmetric=sym)
    check(got, expect(x, ref))
    tie_to_reference_figure(x, ref, got)


@pytest.mark.parametrize("gs", [32, 64, 256])
@pytest.mark.parametrize("dtype,bits,sym", [(torch.bfloat16, 4, False), (torch.float32, 8, True),
                                            (torch.float16, 4, True)])
def test_rtn_group_sizes(gs, dtype, bits, sym):
    _dev()
    x = weights((5, 512), dtype, seed=gs)
    q = quantizer(bits, gs, sym)
    got = q.quantization_error(x, q.quantize_packed(x), per_group=True)
    ref = orc.quantize(x, bits=bits, group_size=gs, symmetric=sym)
    check(got, expect(x, ref))
    tie_to_reference_figure(x, ref, got)


def test_without_per_group_returns_numbers_only():
    _dev()
    x = weights((3, 256), torch.bfloat16, seed=1)
    q = quantizer()
    got = q.quantization_error(x, q.quantize_packed(x))
    assert sorted(got) == sorted(["numel", "nonfinite", "sum_abs", "sum_sq", "sum_w_sq", "mean_abs_error", "mse",
                                  "max_abs_error", "snr_db", "input_scaled"])
    assert got["input_scaled"] is False


# ---------------------------------------------------------------- hand-built results
def hand_built(shape, gs, bits, sym, seed, special=True):
    """A result unrelated to any weights: random fields, zero points and fp16 scales."""
    g = torch.Generator().manual_seed(seed)
    rows, K = shape
    G = -(-K // gs)
    qmin, qmax = orc.qrange(bits, sym)
    sc = (torch.rand(rows, G, generator=g) * 0.02 + 1e-4).to(torch.float16)
    if special:
        flat = sc.view(-1)
        flat[0] = float("inf")
        flat[1 % flat.numel()] = float("nan")
        flat[2 % flat.numel()] = 0.0
        flat[-1] = 6.0e-8                                 # an fp16 subnormal
    return {"tensor_q": torch.randint(qmin, qmax + 1, (rows, K), generator=g, dtype=torch.int32),
            "scales": sc, "zero_points": torch.randint(qmin, qmax + 1, (rows, G), generator=g, dtype=torch.int32),
            "bits": torch.tensor(bits, dtype=torch.int32), "group_size": torch.tensor(gs, dtype=torch.int32),
            "symmetric": torch.tensor(sym, dtype=torch.bool)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("bits,sym", [(4, False), (4, True), (8, False), (8, True)])
def test_hand_built_results_are_read_not_requantized(dtype, bits, sym):
    _dev()
    x = weights((6, 640), dtype, seed=11)
    ref = hand_built((6, 640), 128, bits, sym, seed=bits + sym)
    want = expect(x, ref)
    assert want["totals"][4] >= 2 * 128                  # the inf- and the NaN-scaled group (scale 0: dq = 0)
    q = quantizer(bits, 128, sym)
    check(q.quantization_error(x, packed_of(ref, (6, 640)), per_group=True), want)
    check(q.quantization_error(x, ref, per_group=True), want)


# ---------------------------------------------------------------- generic path
@pytest.mark.parametrize("shape,gs", [((4, 250), 100), ((3, 100), 24), ((2, 1024), 512), ((4, 130), 128),
                                      ((3, 1000), 512)])
@pytest.mark.parametrize("dtype,bits,sym", [(torch.bfloat16, 4, False), (torch.float16, 8, True),
                                            (torch.float32, 4, True), (torch.float32, 8, False)])
def test_generic_path(shape, gs, dtype, bits, sym):
    _dev()
    x = weights(shape, dtype, seed=gs)
    q = quantizer(bits, gs, sym)
    got = q.quantization_error(x, q.quantize_packed(x), per_group=True)
    ref = orc.quantize(x, bits=bits, group_size=gs, symmetric=sym)
    check(got, expect(x, ref))
    tie_to_reference_figure(x, ref, got)
    hb = hand_built(shape, gs, bits, sym, seed=gs + bits)
    check(q.quantization_error(x, hb, per_group=True), expect(x, hb))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("bits", [4, 8])
def test_both_kernels_agree_aligned_and_unaligned(dtype, bits):
    """gs 128 at [8, 512] is eligible for the streaming kernel; the same weights one element off
    16-B alignment take the generic kernel.  Same bits, and the expectation's."""
    dev = _dev()
    from awq_quantizer import _hip
    x = weights((8, 512), dtype, seed=3)
    ref = hand_built((8, 512), 128, bits, False, seed=9, special=False)
    pk = {k: v.to(dev) for k, v in packed_of(ref, (8, 512)).items()}
    base = torch.empty(8 * 512 + 8, dtype=dtype, device=dev)
    outs = []
    for off in (0, 1, 8 if dtype == torch.bfloat16 else 4):     # aligned, one element off, 16 B on
        w = base[off:off + 8 * 512].view(8, 512)
        w.copy_(x)
        assert (w.data_ptr() % 16 == 0) == (off != 1)
        stats, bad, tot = _hip.quant_error(w, 8, 512, 128, bits, False, pk["qweight"], pk["qzeros"], pk["scales"])
        outs.append((stats.cpu(), bad.cpu(), tot.cpu()))
    for o in outs[1:]:
        assert all(bits_equal(a, b) for a, b in zip(outs[0], o))
    want = expect(x, ref)
    st = outs[1][0].numpy()
    for i, k in enumerate(("group_abs", "group_sq", "group_w_sq", "group_max")):
        assert np.array_equal(st[i].view(np.int32), want[k].reshape(-1).view(np.int32)), k
    assert np.array_equal(outs[1][2].numpy().view(np.int64), want["totals"].view(np.int64))


def test_totals_may_be_left_out():
    dev = _dev()
    from awq_quantizer import _hip
    x = weights((4, 256), torch.bfloat16, seed=2)
    pk = quantizer().quantize_packed(x)
    s0, b0, t0 = _hip.quant_error(x.to(dev), 4, 256, 128, 4, False, pk["qweight"], pk["qzeros"], pk["scales"])
    s1, b1, t1 = _hip.quant_error(x.to(dev), 4, 256, 128, 4, False, pk["qweight"], pk["qzeros"], pk["scales"],
                                  totals=False)
    assert t1 is None and torch.equal(s0.view(torch.int32), s1.view(torch.int32)) and torch.equal(b0, b1)


# ---------------------------------------------------------------- level-2 boundaries
@pytest.mark.parametrize("shape", [(1, 2080), (1, 32800), (257, 4096)])   # 65, 1025, 32 896 groups of 32
def test_level2_boundaries(shape):
    _dev()
    x = weights(shape, torch.bfloat16, seed=shape[1])
    q = quantizer(4, 32, False)
    got = q.quantization_error(x, q.quantize_packed(x), per_group=True)
    ref = orc.quantize(x, bits=4, group_size=32, symmetric=False)
    check(got, expect(x, ref))
    tie_to_reference_figure(x, ref, got)


# ---------------------------------------------------------------- non-finite
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_nonfinite_weights(dtype):
    _dev()
    x = weights((4, 512), dtype, seed=7)
    x[0, 3], x[1, 130], x[2, 511] = float("nan"), float("inf"), float("-inf")
    q = quantizer(4, 128, False)
    # RTN of the poisoned groups (NaN scales), and a finite hand-built result over the same weights
    got = q.quantization_error(x, q.quantize_packed(x), per_group=True)
    want = expect(x, orc.quantize(x, bits=4, group_size=128, symmetric=False))
    assert want["totals"][4] >= 3
    check(got, want)
    hb = hand_built((4, 512), 128, 4, False, seed=21, special=False)
    want = expect(x, hb)
    assert want["totals"][4] == 3 and want["group_nonfinite"][0, 0] == 1
    check(q.quantization_error(x, hb, per_group=True), want)


def test_w_squared_overflows_while_d_is_finite():
    _dev()
    x = weights((2, 256), torch.float32, seed=8)
    x[0, 5], x[1, 200] = 1e30, -1e30
    hb = hand_built((2, 256), 128, 8, True, seed=22, special=False)
    want = expect(x, hb)
    assert want["totals"][4] == 2 and np.isfinite(want["totals"][:4]).all()
    check(quantizer(8, 128, True).quantization_error(x, hb, per_group=True), want)


def test_every_element_nonfinite():
    _dev()
    x = torch.full((3, 256), float("nan"), dtype=torch.bfloat16)
    q = quantizer(4, 128, False)
    got = q.quantization_error(x, q.quantize_packed(x), per_group=True)
    check(got, expect(x, orc.quantize(x, bits=4, group_size=128, symmetric=False)))
    assert got["nonfinite"] == got["numel"] == 768
    assert (got["sum_abs"], got["sum_sq"], got["sum_w_sq"], got["max_abs_error"]) == (0.0, 0.0, 0.0, 0.0)
    assert math.isnan(got["mean_abs_error"])


# ---------------------------------------------------------------- dict formats, model, verify
def test_reference_format_dict_gives_the_packed_dicts_bits():
    _dev()
    x = weights((17, 384), torch.float16, seed=4)
    for bits, sym in ((4, False), (8, True)):
        q = quantizer(bits, 128, sym)
        a = q.quantization_error(x, q.quantize_packed(x), per_group=True)
        b = q.quantization_error(x, q.quantize(x), per_group=True)
        for k, v in a.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v.view(torch.int32), b[k].view(torch.int32)), k
            else:
                assert v == b[k], k


def test_quantization_error_model_skips_and_logs():
    _dev()
    q = quantizer()
    tensors = {"a": weights((4, 256), torch.bfloat16, 1), "b": weights((2, 128), torch.float16, 2),
               "small": weights((16,), torch.float32, 3)}
    results = q.quantize_model(tensors)
    results["ghost"] = results["a"]
    out = q.quantization_error_model(tensors, results)
    assert sorted(out) == ["a", "b"]                       # small-tensor result and the sourceless one skipped
    assert out["a"] == q.quantization_error(tensors["a"], results["a"])


# ---------------------------------------------------------------- activation-aware results (input_scale)
def _act_inputs(dtype):
    g = torch.Generator().manual_seed(13)
    ws = {"q_proj.weight": weights((64, 256), dtype, 31), "k_proj.weight": weights((24, 256), dtype, 32)}
    x = (torch.randn(96, 256, generator=g) * (1 + 20 * (torch.rand(256, generator=g) < 0.05))).to(dtype)
    return ws, x


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_layer_group_results_are_measured_against_the_scaled_weights(dtype):
    """quantize_layer_group results quantize W * diag(input_scale): the report is taken against
    RN_D(W * input_scale) (orc.apply_input_scale), not against W."""
    from awq_quantizer.quantization import AWQQuantizer
    _dev()
    q = AWQQuantizer(bits=4, group_size=128, symmetric=False, scale_method="awq", search_grid=8, device="cuda:0",
                     logger_level="ERROR")
    ws, x = _act_inputs(dtype)
    ref_out = q.quantize_layer_group(ws, x, packed=False)
    pk_out = q.quantize_layer_group(ws, x, packed=True)
    s = ref_out["input_scale"].cpu()
    assert not torch.equal(s, torch.ones_like(s))         # the search moved the channels
    for name, w in ws.items():
        ref = {k: v.cpu() for k, v in ref_out["results"][name].items()}
        assert "input_scale" in ref and "input_scale" in pk_out["results"][name]
        want = expect(orc.apply_input_scale(w, s), ref)
        got = q.quantization_error(w, ref_out["results"][name], per_group=True)
        assert got["input_scaled"] is True
        check(got, want)
        check(q.quantization_error(w, pk_out["results"][name], per_group=True), want)
        plain = dict(ref)
        del plain["input_scale"]                          # the same fields against the unscaled W: another figure
        assert q.quantization_error(w, plain)["sum_sq"] != got["sum_sq"]


@pytest.mark.parametrize("fmt", ["packed", "reference"])
def test_verify_act_stats_checkpoint(tmp_path, fmt):
    """--scale_method awq --act_stats checkpoints: verify scales the source like the checkpoint."""
    _dev()
    from safetensors.torch import save_file
    from awq_quantizer import verify
    from awq_quantizer.main import main
    ws, x = _act_inputs(torch.bfloat16)
    src = tmp_path / "src"
    src.mkdir()
    save_file(ws, str(src / "model.safetensors"))
    xm, xs = orc.act_stats(x)
    stats = str(tmp_path / "stats.safetensors")
    save_file({"q_proj.weight.x_mean": xm, "q_proj.weight.x_sq": xs}, stats)
    out = tmp_path / "out"
    assert main(["--model_id", str(src), "--output_dir", str(out), "--scale_method", "awq", "--act_stats", stats,
                 "--search_grid", "8", "--output_format", fmt, "--log_level", "ERROR"]) == 0
    assert verify.main(["--model_id", str(src), "--quantized_dir", str(out), "--log_level", "ERROR"]) == 0
    rep = json.load(open(out / "quantization_error.json"))
    results = dict(verify.iter_results(str(out)))
    assert "input_scale" in results["q_proj.weight"] and "input_scale" not in results["k_proj.weight"]
    assert rep["tensors"]["q_proj.weight"]["input_scaled"] is True
    assert rep["tensors"]["k_proj.weight"]["input_scaled"] is False
    if fmt == "reference":
        for name, w in ws.items():
            res = results[name]
            src_w = orc.apply_input_scale(w, res["input_scale"]) if "input_scale" in res else w
            want = expect(src_w, res)
            e = rep["tensors"][name]
            got = np.array([e["sum_abs"], e["sum_sq"], e["sum_w_sq"], e["max_abs_error"], float(e["nonfinite"])])
            assert np.array_equal(got.view(np.int64), want["totals"].view(np.int64)), name
    else:
        q = quantizer(4, 128, False)
        for name, w in ws.items():
            assert rep["tensors"][name] == q.quantization_error(w, results[name]), name


@pytest.mark.parametrize("st", [False, True])
def test_verify_end_to_end(tmp_path, st):
    _dev()
    from safetensors.torch import save_file
    from awq_quantizer import verify
    from awq_quantizer.main import main
    tensors = {"model.layers.0.q_proj.weight": weights((64, 256), torch.bfloat16, 1),
               "lm_head.weight": weights((8, 384), torch.float16, 2)}
    src = tmp_path / "src"
    src.mkdir()
    save_file(tensors, str(src / "model.safetensors"))
    reports = {}
    for fmt in ("packed", None):
        out = tmp_path / f"out_{fmt}"
        argv = ["--model_id", str(src), "--output_dir", str(out), "--log_level", "ERROR"]
        argv += ["--output_format", fmt] if fmt else []
        assert main(argv + (["--save_safetensors"] if st else [])) == 0
        assert verify.main(["--model_id", str(src), "--quantized_dir", str(out), "--log_level", "ERROR"]) == 0
        rep = json.load(open(out / "quantization_error.json"))
        assert set(rep["tensors"]) == set(tensors) and not rep["problems"]
        q = quantizer(4, 128, True)
        for name, res in verify.iter_results(str(out)):
            assert ("qweight" in res) == (fmt == "packed")
            assert rep["tensors"][name] == q.quantization_error(tensors[name], res), name
        assert rep["totals"]["numel"] == 64 * 256 + 8 * 384
        assert rep["totals"]["sum_sq"] == math.fsum(e["sum_sq"] for e in rep["tensors"].values())
        reports[fmt] = rep
    assert reports["packed"]["tensors"] == reports[None]["tensors"]
