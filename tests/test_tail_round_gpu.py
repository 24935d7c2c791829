"""awq_gptq_round_block (csrc/awq_gptq_round.hip) and AWQQuantizer.quantize_gptq on the GPU, against
the NumPy restatement tests/gptq_round_ref.py.

The kernel, bit for bit.  Every case runs out of a guard-band arena (tests/guard_arena.py through
test_gpu_bounds.Call), from the fill and from its complement: qweight, the scale bits, err and the
updated work are compared with the float32 restatement byte for byte, the words and scales of other
blocks must keep the fill, and qzeros — a read-modify-write of the block's zero FIELDS — starts
from random words whose other fields must come back unchanged.  Shapes: N = 1 (one lane), 70 (a
partial second wave), 130 (more than two waves; one workgroup per 64 rows, the grid is not capped,
so there is no later loop trip to reach); K = 256 with col_begin 0 and 128, K = 192 with a
64-column last block at group size 32 and 64; group size 32 / 64 / 128; 4 and 8 bits; both
symmetries.  With N >= 70, row 3 holds a constant group, row 5 an all-zero group and row 7 a NaN;
the restatement's rows do not meet, so equality with it shows the finite rows unaffected.

quantize_gptq.  loss / loss64 is the output error of the GPU result over that of the float64
restatement on the same inputs.  Measured on an MI355X over seeds 0..4 of the three shapes, bf16 and
fp16 (30 runs): 0.9943 .. 1.0009, worst 1.0009 (N 32, K 256, T 128, bf16, seed 0).  The fp32 solver
is not worse than the float64 one: the two differ by the few rounding decisions that the fp32
X^T X, the fp32 Cholesky factorisations and the trailing GEMMs' summation order move, in either
direction, by up to 0.6 %.  LOSS_BOUND = 1.02 is the worst seed plus three times that spread, as
headroom for another library's summation order.
"""
import numpy as np
import pytest
import torch

import gptq_round_ref as gr
from test_gpu_bounds import BF16, F16, Call, _dev, _lib, _stream, elem_mask

pytestmark = pytest.mark.gpu

_ids = lambda v: str(v).replace("torch.", "")

# (N, K, group size, bits, symmetric, col_begin, n_cols)
KERNEL_CASES = [
    (1, 256, 128, 4, False, 0, 128), (70, 256, 128, 4, False, 128, 128), (130, 256, 64, 4, True, 0, 128),
    (70, 256, 32, 8, False, 128, 128), (130, 256, 32, 4, False, 0, 128), (70, 192, 32, 4, False, 128, 64),
    (70, 192, 64, 8, True, 128, 64), (1, 192, 64, 4, False, 0, 128), (130, 256, 128, 8, True, 0, 128),
    (70, 256, 64, 8, False, 0, 128), (70, 256, 128, 4, True, 128, 128), (130, 256, 32, 8, True, 128, 128),
]
_KREF = {}


def kernel_case(N, K, gs, bits, sym, c0, n):
    """Inputs and the restatement's outputs, once per case."""
    key = (N, K, gs, bits, sym, c0, n)
    if key in _KREF:
        return _KREF[key]
    X, W = gr.inputs(N, K, 300, seed=N + K + gs + bits + c0)
    U = gr.factor(X)[0].astype(np.float32)
    work = W.astype(np.float32)
    if N >= 70:
        work[3, c0:c0 + gs] = 0.25                      # a constant group
        work[5, c0:c0 + gs] = 0.0                       # an all-zero group
        work[7, c0 + 5] = np.nan                        # a NaN
    G, per = K // gs, 32 // bits
    g = np.random.default_rng(N + K)
    fields = g.integers(0, 1 << bits, (N, K))           # what other blocks hold: anything
    zfields = g.integers(0, 1 << bits, (N, -(-G // per) * per))
    sbits = g.integers(0, 1 << 16, (N, G)).astype(np.uint16)
    qz_before = gr.pack_words(zfields, bits)
    after = work.copy()
    zf = zfields[:, :G].copy()
    err = gr.round_block(after, U, gs, bits, sym, c0, n, fields, zf, sbits)
    zfields[:, :G] = zf
    in_block = np.zeros((N, K), bool)
    in_block[:, c0:c0 + n] = True
    grp_block = np.zeros((N, G), bool)
    grp_block[:, c0 // gs:(c0 + n) // gs] = True
    _KREF[key] = {"work": work, "U": U, "after": after, "err": err, "qweight": gr.pack_words(fields, bits),
                  "qw_mask": gr.pack_words(np.where(in_block, (1 << bits) - 1, 0), bits) != 0,
                  "qz_before": qz_before, "qzeros": gr.pack_words(zfields, bits), "sbits": sbits,
                  "s_mask": grp_block}
    return _KREF[key]


@pytest.mark.parametrize("N,K,gs,bits,sym,c0,n", KERNEL_CASES, ids=_ids)
def test_kernel_bit_for_bit(N, K, gs, bits, sym, c0, n):
    dev = _dev()
    r = kernel_case(N, K, gs, bits, sym, c0, n)
    if N >= 70:                                         # the crafted rows are what they are meant to be
        g0, g1 = c0 // gs, (c0 + n) // gs - 1
        assert r["sbits"][5, g0] == 0 and not r["err"][5, :gs].any() and g1 >= g0
        if not sym:                                     # (symmetric: the range [-0.25, 0.25] is a regular group)
            assert r["sbits"][3, g0] == 0 and not r["err"][3, :gs].any()
        assert r["sbits"][7, g0] == 0xFFFF and not r["err"][7, :gs].any() and np.isnan(r["after"][7, c0 + 5])
        assert r["err"][0].any() and r["err"][5, gs:].any() == (n > gs)
    c = Call(dev, seed=N + K + gs + c0)
    wb = c.inp("work", torch.from_numpy(r["work"]), expect=torch.from_numpy(r["after"]), untouched=False,
               nan_dtype=torch.float32)
    ub = c.inp("u", torch.from_numpy(r["U"]))
    eb = c.out("err", torch.from_numpy(r["err"]))
    qw = c.out("qweight", torch.from_numpy(r["qweight"]), written=elem_mask(torch.from_numpy(r["qw_mask"]), 4))
    qz = c.inp("qzeros", torch.from_numpy(r["qz_before"]), expect=torch.from_numpy(r["qzeros"]), untouched=False)
    sc = c.out("scales", torch.from_numpy(r["sbits"].view(np.int16)), written=elem_mask(torch.from_numpy(r["s_mask"]), 2))
    c.build()
    c.run(lambda: _lib().awq_gptq_round_block(wb.ptr, N, K, gs, bits, int(sym), ub.ptr, c0, n, eb.ptr, qw.ptr, qz.ptr,
                                              sc.ptr, _stream(dev)))


def test_order_round_block():
    """The entry on a non-blocking stream behind tests/stream_gate.py's gate: one lane, three
    workgroups, a short last block."""
    from test_stream_order_gpu import walk
    walk([("gptq_round_block one row", test_kernel_bit_for_bit, KERNEL_CASES[0]),
          ("gptq_round_block 130 rows sym", test_kernel_bit_for_bit, KERNEL_CASES[2]),
          ("gptq_round_block 64-column block", test_kernel_bit_for_bit, KERNEL_CASES[5])])


# ---------------------------------------------------------------- quantize_gptq
SHAPES = [(32, 256, 512, 128), (32, 256, 128, 128), (16, 384, 300, 64)]       # (N, K, T, group size)
SEEDS = range(5)
MEASURED_WORST = 1.0009   # loss / loss64, the worst of SHAPES x {bf16, fp16} x SEEDS on an MI355X
LOSS_BOUND = 1.02         # the module docstring says how it is set
_QREF = {}


def quantizer(gs, sym=False, bits=4):
    from awq_quantizer.quantization import AWQQuantizer
    return AWQQuantizer(bits=bits, group_size=gs, symmetric=sym, device="cuda:0", logger_level="ERROR")


def gptq_case(N, K, T, gs, dtype, seed):
    """The inputs rounded to dtype, the float64 restatement's loss on them and round-to-nearest's."""
    key = (N, K, T, gs, dtype, seed)
    if key not in _QREF:
        X, W = gr.inputs(N, K, T, seed)
        x, w = torch.from_numpy(X).to(dtype), torch.from_numpy(W).to(dtype)
        Xd, Wd = x.double().numpy(), w.double().numpy()
        U, dead = gr.factor(Xd)
        ref = gr.solve(Wd, U, gs, 4, False, dtype=np.float64, dead=dead)
        _QREF[key] = {"x": x, "w": w, "X": Xd, "W": Wd, "loss64": gr.output_loss(gr.dequantize(ref, gs), Wd, Xd)}
    return _QREF[key]


def reported_loss_is_the_results(q, packed, got, W, X):
    """A reported loss is the output error of what dequantize_packed gives, within
    awq_output_error's contract: |E - E_exact| <= (2^-17 + K 2^-22) sum_k |d| |x| per output, and
    (T + 1) 2^-24 relative on the sum of squares.  -> the float64 value."""
    dq = q.dequantize_packed(packed).double().cpu().numpy()
    D = dq - W
    E = D @ X.T
    exact = float((E * E).sum())
    K, T = W.shape[1], X.shape[0]
    b = (2.0 ** -17 + K * 2.0 ** -22) * (np.abs(D) @ np.abs(X).T)
    slack = float((2 * np.abs(E) * b + b * b).sum()) + (T + 1) * 2.0 ** -24 * exact
    assert abs(got - exact) <= slack, (got, exact, slack)
    return exact


@pytest.mark.parametrize("dtype", [BF16, F16], ids=_ids)
@pytest.mark.parametrize("N,K,T,gs", SHAPES, ids=_ids)
def test_quantize_gptq_loss(N, K, T, gs, dtype):
    _dev()
    q = quantizer(gs)
    worst = 0.0
    for seed in SEEDS:
        c = gptq_case(N, K, T, gs, dtype, seed)
        r = q.quantize_gptq(c["w"], c["x"])
        rd = r["rounding"]
        assert rd["fallback"] is False and rd["damp"] == 0.01 and rd["dead_columns"] == 0      # T < K included
        assert tuple(r["shape"].tolist()) == (N, K) and r["qweight"].is_cuda
        exact = reported_loss_is_the_results(q, r, rd["loss"], c["W"], c["X"])
        reported_loss_is_the_results(q, q.quantize_packed(c["w"].to("cuda:0")), rd["loss_rtn"], c["W"], c["X"])
        ratio = exact / c["loss64"]
        worst = max(worst, ratio)
        print(f"quantize_gptq N {N} K {K} T {T} gs {gs} {_ids(dtype)} seed {seed}: loss / loss_rtn "
              f"{rd['loss'] / rd['loss_rtn']:.4f}  loss / loss64 {ratio:.4f}")
        assert rd["loss"] < rd["loss_rtn"]
        assert ratio <= LOSS_BOUND
    print(f"worst loss / loss64 N {N} K {K} T {T} gs {gs} {_ids(dtype)}: {worst:.4f} (bound {LOSS_BOUND})")


@pytest.mark.parametrize("sym,bits", [(False, 4), (True, 4), (False, 8)], ids=_ids)
def test_input_scale_is_the_hand_made_composition(sym, bits):
    """quantize_gptq(w, x, input_scale=s) == quantize_gptq(RN(w s), fp32(x) RN(1 / s)), bit for bit."""
    from awq_quantizer import _hip
    dev = _dev()
    c = gptq_case(32, 256, 512, 128, BF16, 1)
    q = quantizer(128, sym, bits)
    s = torch.exp(0.3 * torch.randn(256, generator=torch.Generator().manual_seed(5))).to(dev)
    got = q.quantize_gptq(c["w"], c["x"], input_scale=s)
    w = c["w"].to(dev)
    hand = q.quantize_gptq(_hip.apply_input_scale(w, s),
                           c["x"].to(dev).float() * _hip.act_recip_table(s.reshape(1, -1)).reshape(-1))
    for k in ("qweight", "qzeros"):
        assert torch.equal(got[k], hand[k]), k
    assert torch.equal(got["scales"].view(torch.int16), hand["scales"].view(torch.int16))
    assert torch.equal(got["input_scale"], s) and "input_scale" not in hand
    assert got["rounding"]["loss"] < got["rounding"]["loss_rtn"]
    plain = q.quantize_gptq(c["w"], c["x"])
    assert not torch.equal(got["qweight"], plain["qweight"])


@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
def test_dead_columns_encode_zero(sym):
    _dev()
    c = gptq_case(16, 384, 300, 64, BF16, 2)
    x = c["x"].clone()
    dead = [3, 64, 200]
    x[:, dead] = 0
    q = quantizer(64, sym)
    r = q.quantize_gptq(c["w"], x)
    assert r["rounding"]["dead_columns"] == len(dead) and r["rounding"]["fallback"] is False
    dq = q.dequantize_packed(r).cpu()
    assert bool((dq[:, dead] == 0).all()) and bool((dq != 0).any(dim=0).sum() > 300)
    assert r["rounding"]["loss"] < r["rounding"]["loss_rtn"]


def test_hessian_argument_and_fallbacks():
    dev = _dev()
    c = gptq_case(32, 256, 512, 128, BF16, 0)
    q = quantizer(128)
    ref = q.quantize_gptq(c["w"], c["x"])
    H = c["x"].to(dev).float().t() @ c["x"].to(dev).float()
    r = q.quantize_gptq(c["w"], hessian=H)                       # the Hessian alone: the same bits, no report
    assert torch.equal(r["qweight"], ref["qweight"]) and r["rounding"]["loss"] is None and r["rounding"]["loss_rtn"] is None
    rtn = q.quantize_packed(c["w"].to(dev))
    bad = c["w"].clone()
    bad[2, 7] = float("inf")
    f = q.quantize_gptq(bad, c["x"])                             # a non-finite weight: quantize_packed's result
    assert f["rounding"]["fallback"] is True
    assert torch.equal(f["qweight"], q.quantize_packed(bad.to(dev))["qweight"])
    f = q.quantize_gptq(c["w"], hessian=-torch.eye(256))         # not positive definite: three tries, then the fallback
    assert f["rounding"]["fallback"] is True and f["rounding"]["damp"] == pytest.approx(1.0)
    assert torch.equal(f["qweight"], rtn["qweight"]) and torch.equal(f["qzeros"], rtn["qzeros"])


def test_layer_group_mode():
    """q.rounding = "gptq": a group with samples goes through quantize_gptq with the searched scale;
    one without rounds to nearest."""
    dev = _dev()
    from awq_quantizer.quantization import AWQQuantizer
    c = gptq_case(32, 256, 512, 128, BF16, 3)
    q = AWQQuantizer(bits=4, group_size=128, symmetric=False, device="cuda:0", scale_method="awq", logger_level="ERROR")
    weights = {"a": c["w"], "b": c["w"].flip(0).contiguous()}
    near = q.quantize_layer_group(weights, c["x"])
    q.rounding = "gptq"
    out = q.quantize_layer_group(weights, c["x"])
    assert torch.equal(out["input_scale"], near["input_scale"]) and out["best"] == near["best"]
    for name, w in weights.items():
        r = out["results"][name]
        hand = q.quantize_gptq(w, c["x"], input_scale=out["input_scale"], damp=q.gptq_damp)
        assert torch.equal(r["qweight"], hand["qweight"]) and torch.equal(r["qzeros"], hand["qzeros"])
        assert not torch.equal(r["qweight"], near["results"][name]["qweight"])
        assert r["rounding"]["loss"] < r["rounding"]["loss_rtn"]
    stats = q.quantize_layer_group(weights, x_mean=c["x"].float().abs().mean(0), x_sq=(c["x"].float() ** 2).mean(0))
    for name in weights:                                          # statistics only: no samples, nearest
        assert "rounding" not in stats["results"][name]
