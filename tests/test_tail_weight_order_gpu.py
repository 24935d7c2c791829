"""GPTQ act-order (csrc/awq_gptq_actorder.hip) on the GPU against tests/gptq_layout.py,
tests/gptq_reader.py and the float64 solver of tests/gptq_round_ref.py.  Shapes (N, K, group size):
(8, 64, 32) one qzeros word, one strip; (72, 256, 128) N off the 64-word strip and the 64-row tile;
(136, 640, 64) 80 word rows (a second 64-row chunk of the gather), five dequantize tiles along K.
The solver's loss is re-measured with gptq_reader's float64 weights rounded to fp16 once: the
arithmetic awq_output_error documents for its dq (the reader's unrounded product is not)."""
import numpy as np
import pytest
import torch

import gptq_layout as gl
import gptq_reader
import gptq_round_ref as gr
from test_gpu_bounds import BF16, F16, F32, Call, _dev, _lib, _stream
from test_serving_gptq_gpu import FORMATS, bits16, packed, quantizer, same
from test_tail_round_gpu import LOSS_BOUND, gptq_case

pytestmark = pytest.mark.gpu

SHAPES = [(8, 64, 32), (72, 256, 128), (136, 640, 64)]
PARTS = ("qweight", "qzeros", "scales", "g_idx")
_ids = lambda v: str(v).replace("torch.", "")


def perm_of(kind, K):
    if kind == "identity":
        return torch.arange(K)
    return torch.arange(K).flip(0) if kind == "reversal" else torch.randperm(K, generator=torch.Generator().manual_seed(K))


def act_order_layout(pc, perm, gs, off):
    """The CPU restatement: pc's fields are in permuted order; column perm[i] of the layout is field
    column i, and its group is i // gs."""
    K = perm.numel()
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(K)
    want = gl.pack(gl.fields_of(pc["qweight"], K)[:, inv], gl.fields_of(pc["qzeros"], K // gs), pc["scales"], gs, off)
    return dict(want, g_idx=(inv // gs).to(torch.int32))


@pytest.mark.parametrize("sym,fmt", [(False, "gptq"), (True, "gptq_v2"), (False, "gptq_v2"), (True, "gptq")], ids=_ids)
@pytest.mark.parametrize("kind", ["identity", "reversal", "random"])
@pytest.mark.parametrize("N,K,gs", SHAPES, ids=_ids)
def test_export_import_bit_for_bit(N, K, gs, kind, sym, fmt):
    _dev()
    p, pc = packed(N, K, gs, BF16, sym)
    q, perm = quantizer(gs, sym), perm_of(kind, K)
    got = q.export_gptq(dict(p, perm=perm.to(torch.int32)), fmt)
    same(got, act_order_layout(pc, perm, gs, FORMATS[fmt]), kind)
    if kind == "identity":
        same(got, {k: v.cpu() for k, v in q.export_gptq(p, fmt).items()}, "no perm")
        return
    r = q.import_gptq({k: got[k] for k in PARTS}, checkpoint_format=fmt)
    g = got["g_idx"].cpu().long()
    assert torch.equal(r["perm"].cpu().long(), torch.sort(g, stable=True).indices) and torch.equal(r["shape"], p["shape"])
    same(q.export_gptq(r, fmt), {k: got[k].cpu() for k in PARTS}, "round trip")


def dequant_case(N, K, gs, kind, fmt):
    """(the GPTQ tensors of the crafted result with this g_idx on the CPU, gptq_layout's weight)."""
    _, pc = packed(N, K, gs, BF16, False)
    t = gl.from_packed(pc, FORMATS[fmt])
    G, g = K // gs, torch.Generator().manual_seed(N + K)
    t["g_idx"] = {"balanced": lambda: t["g_idx"][torch.randperm(K, generator=g)],
                  "zeros": lambda: torch.zeros(K, dtype=torch.int32),
                  "random": lambda: torch.randint(0, G, (K,), generator=g, dtype=torch.int32),
                  "trivial": lambda: t["g_idx"]}[kind]()
    return t, gl.dequantize(t, FORMATS[fmt])


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("kind", ["balanced", "zeros", "random", "trivial"])
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=_ids)
@pytest.mark.parametrize("N,K,gs", SHAPES, ids=_ids)
def test_fused_dequantize_exact(N, K, gs, dtype, kind, fmt):
    from awq_quantizer import _hip
    dev = _dev()
    t, ref = dequant_case(N, K, gs, kind, fmt)
    assert bool(torch.isfinite(ref).all())
    d = {k: v.to(dev) for k, v in t.items()}
    out = torch.empty((N, K), dtype=dtype, device=dev)
    _hip.dequantize_gptq(d["qweight"], d["qzeros"], d["scales"], d["g_idx"], FORMATS[fmt], out)
    view = (lambda x: x.cpu().view(torch.int32)) if dtype == F32 else bits16
    assert torch.equal(view(out), view(ref.to(dtype)))
    via = quantizer(gs).dequantize_gptq(d, checkpoint_format=fmt, dtype=dtype)      # the public route picks it
    assert torch.equal(view(via), view(out))
    if kind == "trivial":                           # ... and today's route gives the same bits
        today = quantizer(gs).dequantize_packed(quantizer(gs).import_gptq(d, checkpoint_format=fmt), dtype)
        assert torch.equal(view(today), view(out))


# ---------------------------------------------------------------- the entries out of a guard-band arena
ARENA = [("permute", 136, 640, 64, 0), ("permute", 136, 640, 64, 4), ("gidx", 8, 640, 64, 0),
         ("dequant", 72, 256, 128, 0), ("dequant", 136, 640, 64, 2)]


@pytest.mark.parametrize("entry,N,K,gs,skew", ARENA, ids=_ids)
def test_entry_guard_bands(entry, N, K, gs, skew):
    """Every output exactly its size, from the fill and from its complement; skew: the pointers that
    many bytes past 16-B alignment (the element paths).  The gather's src holds two entries outside
    [0, K), which take field 0; index inputs stay real in ordered mode."""
    dev = _dev()
    t, ref = dequant_case(N, K, gs, "balanced", "gptq")
    perm = perm_of("random", K).to(torch.int32)
    c = Call(dev, seed=N + K + skew)
    if entry == "permute":
        src = perm.clone()
        src[5], src[K - 1] = K, -1
        u = gl.unpack(t, 1)[0][:, torch.where((src < 0) | (src >= K), 0, src).long()]
        want = gl.pack(u, *gl.unpack(t, 1)[1:], gs, 1)["qweight"]
        a, s, o = c.inp("in", t["qweight"], skew=skew), c.inp("src", src, pointers=True), c.out("out", want, skew=skew)
        launch = lambda: _lib().awq_gptq_permute_rows(a.ptr, s.ptr, N, K, o.ptr, _stream(dev))
    elif entry == "gidx":
        inv = torch.empty_like(perm)
        inv[perm.long()] = torch.arange(K, dtype=torch.int32)
        s, o, i = c.inp("perm", perm, pointers=True), c.out("g_idx", inv // gs), c.out("invperm", inv)
        launch = lambda: _lib().awq_gptq_gidx_from_perm(s.ptr, K, gs, o.ptr, i.ptr, _stream(dev))
    else:
        ins = [c.inp(k, t[k], pointers=k == "g_idx") for k in PARTS]
        o = c.out("out", ref.to(BF16), skew=skew)
        launch = lambda: _lib().awq_dequantize_gptq(ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, N, K, K // gs, 1,
                                                    o.ptr, 0, _stream(dev))
    c.run(launch)


def test_order_act_order_entries():
    """The three entries on a non-blocking stream behind tests/stream_gate.py's gate."""
    from test_stream_order_gpu import walk
    walk([(f"gptq act-order {a[0]}", test_entry_guard_bands, a) for a in (ARENA[1], ARENA[2], ARENA[4])])


def test_check_index_reports_the_first_entry_out_of_range():
    from awq_quantizer import _hip
    idx = torch.arange(3000, dtype=torch.int32, device=_dev())
    assert int(_hip.gptq_check_index(idx, 3000)) == 0
    idx[2047], idx[1500] = -1, 3000
    assert int(_hip.gptq_check_index(idx, 3000)) == 1501
    with pytest.raises(ValueError, match="not a permutation"):
        quantizer(32).export_gptq(dict(packed(8, 64, 32, BF16, False)[0], perm=torch.zeros(64, dtype=torch.int32)))


# ---------------------------------------------------------------- the solver
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_ids)
@pytest.mark.parametrize("N,K,T,gs", [(32, 256, 512, 128), (16, 384, 300, 64)], ids=_ids)
def test_quantize_gptq_act_order(N, K, T, gs, dtype):
    _dev()
    c = gptq_case(N, K, T, gs, dtype, 0)
    H = c["x"].float().t() @ c["x"].float()                       # on the CPU: perm does not hang on a GEMM's order
    diag = H.diagonal()
    assert diag.unique().numel() == K
    perm = torch.argsort(diag, descending=True, stable=True)
    q = quantizer(gs)
    r = q.quantize_gptq(c["w"], c["x"], hessian=H, act_order=True)
    rd = r["rounding"]
    assert torch.equal(r["perm"].cpu().long(), perm) and rd["act_order"] is True and rd["fallback"] is False
    Wp, Xp = c["W"][:, perm.numpy()], c["X"][:, perm.numpy()]
    U, dead = gr.factor(Xp)
    loss64 = gr.output_loss(gr.dequantize(gr.solve(Wp, U, gs, 4, False, dtype=np.float64, dead=dead), gs), Wp, Xp)
    # the loss, measured again from the exported checkpoint by the independent reader
    g = {k: v.cpu() for k, v in q.export_gptq(r).items()}
    dq = gptq_reader.dequant_gptq(g["qweight"], g["qzeros"], g["scales"], g["g_idx"], 1).half().double().numpy()
    assert np.array_equal(dq, q.dequantize_packed(r).double().cpu().numpy())
    D = dq - c["W"]
    E = D @ c["X"].T
    exact = float((E * E).sum())
    b = (2.0 ** -17 + K * 2.0 ** -22) * (np.abs(D) @ np.abs(c["X"]).T)   # awq_output_error's contract, as
    slack = float((2 * np.abs(E) * b + b * b).sum()) + (T + 1) * 2.0 ** -24 * exact   # test_tail_round_gpu.py states it
    print(f"act-order N {N} K {K} T {T} gs {gs} {_ids(dtype)}: loss / loss_rtn {rd['loss'] / rd['loss_rtn']:.4f}  "
          f"loss / loss64 {exact / loss64:.4f}")
    assert abs(rd["loss"] - exact) <= slack, (rd["loss"], exact, slack)
    assert exact / loss64 <= LOSS_BOUND and rd["loss"] < rd["loss_rtn"]
    e = q.quantization_error(c["w"], r, samples=c["x"])
    assert abs(e["output_sum_sq"] - exact) <= slack
    bad = q.quantize_gptq(c["w"], c["x"], hessian=torch.full_like(H, float("nan")), act_order=True)
    assert "perm" not in bad and bad["rounding"]["fallback"] is True
