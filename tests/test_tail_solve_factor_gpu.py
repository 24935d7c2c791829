"""awq_gptq_factor (csrc/awq_gptq_factor.hip) and quantize_gptq with q.gptq_factor = "hip" on the GPU
(DESIGN.md §5.19).

Two figures in float64 against the float64 factor (tests/gptq_round_ref.factor): dU = |U - U64|_F /
|U64|_F and res = |U H_d U^T - I|_F / sqrt(K), each bounded by MARGIN times the same figure of the
three-call torch route on the same fp32 H.  Measured on an MI355X, new / torch over seeds 0..4 of CASES:
dU 0.577 .. 1.366, res 0.474 .. 1.171 (both worst at K 256 seed 0; largest spread over a case's seeds
0.712 and 0.655, K 32).  MARGIN = 3.5 = 1.366 + 3 x 0.712: worst ratio plus three times the spread,
LOSS_BOUND's rule.  Worst loss / loss64 of quantize_gptq with the factor 1.0010; CLI loss / loss_rtn 0.4016.
"""
import numpy as np
import pytest
import torch

import gptq_round_ref as gr
from test_gpu_bounds import BF16, F16, Call, _dev, _lib, _stream
from test_tail_round_gpu import LOSS_BOUND, SHAPES, gptq_case, quantizer, reported_loss_is_the_results
from test_tail_round_model_gpu import LINE, TOKENS, runs  # noqa: F401  (runs: the module-scoped fixture)

pytestmark = pytest.mark.gpu

# (K, T): a partial block; a full one; a ragged second; two, T < K; three; three and a 32-wide one, T < K
CASES = [(32, 64), (128, 300), (192, 300), (256, 128), (384, 300), (416, 100)]
SEEDS = range(5)
MARGIN = 3.5
DAMP = 0.01
_REF = {}


def factor_case(K, T, seed):
    """H on the device (fp32, bf16-rounded samples), U64 and H_d in float64, the torch route's figures."""
    key = (K, T, seed)
    if key not in _REF:
        from awq_quantizer.quantization.gptq_round import _factor
        X, _ = gr.inputs(1, K, T, seed)
        x = torch.from_numpy(X).to(BF16)
        xd = x.to("cuda:0").float()
        H = xd.t() @ xd
        Xd = x.double().numpy()
        Hd = Xd.T @ Xd
        Hd[np.diag_indices(K)] += DAMP * np.mean(np.diag(Hd))
        c = {"H": H, "U64": gr.factor(Xd, DAMP)[0], "Hd": Hd}
        c["torch"] = figures(_factor(H, DAMP), c)
        _REF[key] = c
    return _REF[key]


def figures(U, c):
    U = U.double().cpu().numpy()
    return (float(np.linalg.norm(U - c["U64"]) / np.linalg.norm(c["U64"])),
            float(np.linalg.norm(U @ c["Hd"] @ U.T - np.eye(len(U))) / np.sqrt(len(U))))


def hip_factor(H, damp=DAMP):
    """The entry on a copy of H whose strict lower triangle holds a fill (it is not read)."""
    from awq_quantizer import _hip
    U, status = _hip.gptq_factor(H.triu() + torch.full_like(H, 7.0).tril(-1), damp)
    return U, int(status)


@pytest.mark.parametrize("K,T", CASES, ids=str)
def test_factor_against_float64(K, T):
    _dev()
    for seed in SEEDS:
        c = factor_case(K, T, seed)
        U, status = hip_factor(c["H"])
        assert status == 0
        assert not bool(U.tril(-1).any()) and bool((U.diagonal() > 0).all()) and bool(torch.isfinite(U).all())
        got = figures(U, c)
        print(f"factor K {K} T {T} seed {seed}: {got} ratios {got[0] / c['torch'][0]:.3f} {got[1] / c['torch'][1]:.3f}")
        assert got[0] <= MARGIN * c["torch"][0] and got[1] <= MARGIN * c["torch"][1]


@pytest.mark.parametrize("col", [200, 50], ids=["last block", "first block"])
def test_failure_is_a_status(col):
    """An indefinite H: the status names the column, the same buffers then serve a valid call, and
    quantize_gptq falls back after its retries."""
    from awq_quantizer import _hip
    dev = _dev()
    K = 256
    bad = torch.eye(K, device=dev)
    bad[col, col] = -1.0
    h = bad.clone()
    work = torch.empty(int(_lib().awq_gptq_factor_workspace(K)) // 8, dtype=torch.float64, device=dev)
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    call = lambda: _lib().awq_gptq_factor(_hip.ptr(h), K, DAMP, _hip.ptr(work), work.numel() * 8, _hip.ptr(status),
                                          _stream(dev))
    assert call() == 0 and int(status) == 1 + col
    c = factor_case(K, 128, 0)
    h.copy_(c["H"])
    assert call() == 0 and int(status) == 0
    assert torch.equal(h, hip_factor(c["H"])[0])
    q = quantizer(128)
    q.gptq_factor = "hip"
    r = q.quantize_gptq(gptq_case(32, 256, 128, 128, BF16, 0)["w"], hessian=bad)
    assert r["rounding"]["fallback"] is True and r["rounding"]["factor"] == "hip"
    assert r["rounding"]["damp"] == pytest.approx(1.0)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("N,K,T,gs", SHAPES, ids=str)
def test_quantize_gptq_with_the_hip_factor(N, K, T, gs, dtype):
    _dev()
    q = quantizer(gs)
    q.gptq_factor = "hip"
    worst = 0.0
    for seed in SEEDS:
        c = gptq_case(N, K, T, gs, dtype, seed)
        r = q.quantize_gptq(c["w"], c["x"])
        rd = r["rounding"]
        assert rd["fallback"] is False and rd["factor"] == "hip" and rd["loss"] < rd["loss_rtn"]
        ratio = reported_loss_is_the_results(q, r, rd["loss"], c["W"], c["X"]) / c["loss64"]
        worst = max(worst, ratio)
        assert ratio <= LOSS_BOUND
    print(f"hip factor: worst loss / loss64 N {N} K {K} T {T} gs {gs} {dtype}: {worst:.4f} (bound {LOSS_BOUND})")


def test_bounds():
    """K = 192 out of a guard-band arena, both fills: h rewritten, status written, workspace free."""
    dev = _dev()
    K = 192
    H = factor_case(K, 300, 1)["H"]
    h_in = H.triu() + torch.full_like(H, 7.0).tril(-1)
    U, status = hip_factor(H)
    assert status == 0
    c = Call(dev, seed=K)
    hb = c.inp("h", h_in, expect=U, untouched=False)
    nbytes = int(_lib().awq_gptq_factor_workspace(K))
    wb = c.work("workspace", nbytes)
    sb = c.out("status", torch.zeros(1, dtype=torch.int32))
    c.run(lambda: _lib().awq_gptq_factor(hb.ptr, K, DAMP, wb.ptr, nbytes, sb.ptr, _stream(dev)))


def test_order_factor():
    """The entry on a non-blocking stream behind tests/stream_gate.py's gate."""
    from test_stream_order_gpu import walk
    walk([("gptq_factor K 192", test_bounds, ())])


def test_cli(runs):
    """main --rounding gptq --gptq_factor hip on test_tail_round_model_gpu's llama model and ids: every
    weight's logged loss is below round-to-nearest's, and verify --act_samples accepts the checkpoint."""
    from awq_quantizer import verify
    from awq_quantizer.main import main
    out, log = str(runs["root"] / "hip"), str(runs["root"] / "hip.log")
    assert main(["--model_id", runs["model"], "--device", "cuda:0", "--n_sample_tokens", str(TOKENS), "--group_size", "32",
                 "--output_format", "autoawq", "--scale_method", "awq", "--fold_scales", "--calib_ids",
                 str(runs["root"] / "ids.safetensors"), "--rounding", "gptq", "--gptq_factor", "hip", "--output_dir", out,
                 "--log_file", log]) == 0
    text = open(log).read()
    lines = LINE.findall(text)
    assert {m for m, _, _ in lines} == set(runs["fx"].quantized_names("autoawq")) and "fallback: nearest" not in text
    assert all(float(after) < float(before) for _, before, after in lines), lines
    ratio = sum(float(a) for _, _, a in lines) / sum(float(b) for _, b, _ in lines)
    print(f"--gptq_factor hip: summed logged output error compensated / nearest {ratio:.4f} (torch route: 0.402)")
    assert verify.main(["--model_id", runs["model"], "--quantized_dir", out, "--act_samples", runs["samples"], "--device",
                        "cuda:0", "--log_level", "ERROR"]) == 0
