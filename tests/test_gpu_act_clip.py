"""Activation-aware clip search on the GPU (include/awq_hip.h awq_quantize_clip_scaled,
AWQQuantizer.quantize_layer_group(clip=True), --act_clip), bit for bit against an expectation put
together on the CPU from independent pieces:
  * orc.apply_input_scale gives w' = RN_D(w s);
  * torch min / max give the group ranges, the shrink is two explicit roundings (fp32 product,
    then the dtype);
  * orc.group_params on a [rows G, 2] tensor of the shrunk (mn, mx) pairs with group size 2 gives
    each candidate's exact scale and zero point, orc.apply_params mode 0 its q;
  * dq, d and c are numpy float16 / float32 ops, the group loss is the 8-element chunk loop and the
    pairwise tree restated below;
  * orc.quantize_groups (RTN of w': every group that keeps candidate 0, NaN / inf groups included)
    and orc.pack_rows give the packed words.
int32 words, fp16 scale bits and fp32 loss bits are compared exactly (NaN losses as NaN: the
definition does not pin a NaN's payload)."""
import ctypes
import json

import numpy as np
import pytest
import torch

from oracle import awq_oracle as orc

pytestmark = pytest.mark.gpu
F32, F16 = np.float32, np.float16
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
GRID, CAND = 20, 10


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from awq_quantizer import _hip
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    return dev


# ---------------------------------------------------------------- the expectation (CPU)
def group_sum(v: np.ndarray, gs: int) -> np.ndarray:
    """float32 [R, K] -> the canonical fp32 sum of every group, float32 [R, G]: each 8-element
    chunk in sequence from +0, then the pairwise tree over 64 chunk slots, adjacent pairs first."""
    R, K = v.shape
    G = K // gs
    slots = np.zeros((R, G, 512), dtype=F32)
    slots[:, :, :gs] = v.reshape(R, G, gs)
    slots = slots.reshape(R, G, 64, 8)
    acc = np.zeros((R, G, 64), dtype=F32)
    with np.errstate(all="ignore"):
        for j in range(8):
            acc = (acc + slots[..., j]).astype(F32)
        while acc.shape[-1] > 1:
            acc = (acc[..., 0::2] + acc[..., 1::2]).astype(F32)
    return acc[..., 0]


def expect_clip(w: torch.Tensor, s: torch.Tensor, xs: torch.Tensor, gs: int, bits: int, sym: bool, n_grid: int,
                n_cand: int) -> dict:
    """The definition of include/awq_hip.h (awq_quantize_clip_scaled), step by step."""
    R, K = w.shape
    G = K // gs
    D = w.dtype
    qmin, qmax = orc.qrange(bits, sym)
    wp = orc.apply_input_scale(w, s)                                   # RN_D(w s)
    g3 = wp.float().reshape(R, G, gs)
    mn, mx = g3.min(dim=-1).values, g3.max(dim=-1).values              # torch: NaN propagates
    if sym:                                                            # awq.py:196-199
        a = torch.maximum(mn.abs(), mx.abs())
        mn, mx = -a, a
    w32 = w.float().numpy()
    s32, x32 = s.float().numpy(), xs.float().numpy()
    best = np.full((R, G), np.inf, dtype=F32)
    bi = np.zeros((R, G), dtype=np.int32)
    loss0 = None
    cands = []
    for i in range(n_cand):
        alpha = torch.tensor(F32(n_grid - i) / F32(n_grid), dtype=torch.float32)
        cmn, cmx = (mn * alpha).to(D), (mx * alpha).to(D)              # RN_D(RN_f32(v alpha))
        pairs = torch.stack([cmn.reshape(-1), cmx.reshape(-1)], dim=1).contiguous()
        sc, zp = orc.group_params(pairs, R * G, 2, 2, bits, sym)       # awq.py:202-211, exact values
        sc, zp = sc.reshape(R, G), zp.reshape(R, G)
        q = orc.apply_params(wp, R, K, gs, sc, zp, qmin, qmax, 0).float().numpy()    # awq.py:245-248
        z32 = np.repeat(zp.numpy().astype(F32), gs, axis=1)
        s16 = np.repeat(sc.numpy().astype(F32).astype(F16), gs, axis=1)
        with np.errstate(all="ignore"):
            dq = ((q - z32).astype(F32).astype(F16) * s16).astype(F16)  # fp16(fp16(q - z) fp16(scale))
            d = ((dq.astype(F32) / s32[None, :]).astype(F32) - w32).astype(F32)
            c = (x32[None, :] * (d * d).astype(F32)).astype(F32)
        loss = group_sum(c, gs)
        if i == 0:
            loss0 = loss
        with np.errstate(invalid="ignore"):
            better = loss < best                                       # strict; NaN never wins
        best = np.where(better, loss, best)
        bi = np.where(better, i, bi).astype(np.int32)
        cands.append((np.nan_to_num(q, nan=0.0).astype(np.int32), sc, zp))   # (only finite groups are selected)
    # RTN of w' (candidate 0's outputs, with the reference's NaN / inf conventions)
    tq, sc_out, zp_out = orc.quantize_groups(wp, R, K, gs, bits, sym)
    tq = tq.reshape(R, K).clone()
    sc_out, zp_out = sc_out.clone(), zp_out.clone()
    nan_group = torch.isnan(mn).numpy()
    bi = np.where(nan_group, 0, bi).astype(np.int32)
    for i in range(1, n_cand):
        sel = torch.from_numpy(bi == i)
        if not sel.any():
            continue
        q, sc, zp = cands[i]
        sel_e = sel.repeat_interleave(gs, dim=1)
        tq[sel_e] = torch.from_numpy(q)[sel_e]
        sc_out[sel] = sc.to(torch.float16)[sel]
        zp_out[sel] = zp.to(torch.int32)[sel]
    lossw = np.where(bi == 0, loss0, best).astype(F32)
    return {"qweight": orc.pack_rows(tq, bits, qmin), "qzeros": orc.pack_rows(zp_out, bits, qmin), "scales": sc_out,
            "best_idx": torch.from_numpy(bi.reshape(-1)), "loss": np.stack([loss0.reshape(-1), lossw.reshape(-1)])}


# ---------------------------------------------------------------- inputs and the device call
def weights(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 0.05).to(dtype)


def col_scale(K, seed):
    """log-uniform in [1/4, 4]"""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.exp2(torch.rand(K, generator=g) * 4 - 2).float()


def col_stat(K, seed):
    """x_sq = u^4 + 1e-4, u uniform in [0, 1)"""
    g = torch.Generator().manual_seed(2000 + seed)
    return (torch.rand(K, generator=g) ** 4 + 1e-4).float()


def run_clip(w, s, xs, gs, bits, sym, n_grid=GRID, n_cand=CAND, rscale="table"):
    """The device call through _hip.quantize_clip_scaled; every output as a CPU tensor."""
    from awq_quantizer import _hip
    dev = _dev()
    R, K = w.shape
    G = K // gs
    wd, sd, xd = w.to(dev), s.to(dev), xs.to(dev)
    rs = _hip.act_recip_table(sd.reshape(1, K)).reshape(K) if isinstance(rscale, str) else rscale
    out = {"qweight": torch.full((R, K * bits // 32), -1, dtype=torch.int32, device=dev),
           "qzeros": torch.full((R, -(-G * bits // 32)), -1, dtype=torch.int32, device=dev),
           "scales": torch.full((R, G), -1.0, dtype=torch.float16, device=dev),
           "best_idx": torch.full((R * G,), -1, dtype=torch.int32, device=dev)}
    loss = torch.full((2, R * G), -1.0, dtype=torch.float32, device=dev)
    _hip.quantize_clip_scaled(wd, sd, xd, gs, bits, sym, n_grid, n_cand, rscale=rs, group_loss=loss, **out)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in out.items()}
    got["loss"] = loss.cpu().numpy()
    return got


def assert_same(got: dict, want: dict, what=""):
    for k in ("qweight", "qzeros", "best_idx"):
        assert torch.equal(got[k], want[k]), (what, k)
    assert torch.equal(got["scales"].view(torch.int16), want["scales"].view(torch.int16)), (what, "scales")
    g, e = got["loss"], want["loss"]
    nan = np.isnan(e)
    assert np.array_equal(np.isnan(g), nan), (what, "loss NaN")
    assert np.array_equal(g.view(np.int32)[~nan], e.view(np.int32)[~nan]), (what, "loss")


_EXPECT = {}
# Seeds of the grid cases at group size 256, 4-bit, chosen so that the exact expectation meets
# test_bit_exact_grid's conditions with every dtype.  A tensor has only K / 256 distinct x_sq
# patterns there, and the weighted winner differs from the unweighted one in 5-7 % (symmetric) and
# 9-15 % (asymmetric) of the groups for most seeds: (33, 4096) symmetric reaches 10 % with 3 seeds
# out of 2200 tried.  Every other case takes shape[0] + gs + bits.
_SEEDS_256 = {(False, (5, 512)): 2, (False, (70, 1024)): 4, (False, (9, 3072)): 4, (False, (33, 4096)): 2,
              (True, (5, 512)): 6, (True, (70, 1024)): 31, (True, (9, 3072)): 16, (True, (33, 4096)): 1688}


def grid_case(dtype, gs, bits, sym, shape):
    """Inputs and expectation of one grid case, computed once and shared (never modified)."""
    key = (dtype, gs, bits, sym, shape)
    if key not in _EXPECT:
        seed = _SEEDS_256[(sym, shape)] if (gs, bits) == (256, 4) else shape[0] + gs + bits
        w, s, xs = weights(shape, dtype, seed), col_scale(shape[1], seed), col_stat(shape[1], seed)
        _EXPECT[key] = (w, s, xs, expect_clip(w, s, xs, gs, bits, sym, GRID, CAND))
    return _EXPECT[key]


# ---------------------------------------------------------------- 1. the bit-exact grid
SHAPES = [(5, 512), (70, 1024), (9, 3072), (33, 4096)]   # tiles spanning rows, K < 2048 and K >= 2048 column
                                                         # wraps, a partial last tile


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("bits,sym", [(4, False), (4, True), (8, False)])
@pytest.mark.parametrize("gs", [32, 64, 128, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_exact_grid(dtype, gs, bits, sym, shape):
    _dev()
    w, s, xs, want = grid_case(dtype, gs, bits, sym, shape)
    assert_same(run_clip(w, s, xs, gs, bits, sym), want)
    # the expectation itself must exercise the search (so the comparison cannot pass vacuously)
    bi = want["best_idx"].numpy()
    if bits == 4:
        assert (bi != 0).mean() >= 0.25
        unweighted = expect_clip(w, s, torch.ones_like(xs), gs, bits, sym, GRID, CAND)["best_idx"].numpy()
        assert (bi != unweighted).mean() >= 0.10
    else:
        assert (bi != 0).sum() >= 1


# ---------------------------------------------------------------- 2. identity (a)
@pytest.mark.parametrize("shape", [(5, 512), (9, 3072)])
@pytest.mark.parametrize("gs,bits,sym", [(32, 4, False), (128, 4, True), (256, 8, False), (64, 8, True)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_candidate_is_quantize_groups_scaled(dtype, gs, bits, sym, shape):
    from awq_quantizer import _hip
    dev = _dev()
    seed = gs + shape[0]
    w, s, xs = weights(shape, dtype, seed), col_scale(shape[1], seed), col_stat(shape[1], seed)
    got = run_clip(w, s, xs, gs, bits, sym, n_grid=GRID, n_cand=1)
    R, K = shape
    G = K // gs
    ref = {"qweight": torch.empty((R, K * bits // 32), dtype=torch.int32, device=dev),
           "qzeros": torch.empty((R, -(-G * bits // 32)), dtype=torch.int32, device=dev),
           "scales": torch.empty((R, G), dtype=torch.float16, device=dev)}
    _hip.quantize_groups_scaled(w.to(dev), s.to(dev), gs, bits, sym, **ref)
    for k in ("qweight", "qzeros"):
        assert torch.equal(got[k], ref[k].cpu()), k
    assert torch.equal(got["scales"].view(torch.int16), ref["scales"].cpu().view(torch.int16))
    assert not got["best_idx"].any()
    assert np.array_equal(got["loss"][0].view(np.int32), got["loss"][1].view(np.int32))


# ---------------------------------------------------------------- 3. identity (b)
def _search_case(name):
    dtype = {"bf16": torch.bfloat16, "f32": torch.float32}.get(name, torch.float16)
    w = weights((12, 1024), dtype, seed=len(name))
    if name == "f16_mixed":          # rows 0, 3, 6, 9 with 4-bit scales >= 14 (range / 15): the search kernel's
        w = w.float()                # Markstein chain; the others stay below 14 (its plain chain)
        w[::3] *= 20000.0
        w = w.to(dtype)
    return w


@pytest.mark.parametrize("bits,sym", [(4, False), (4, True), (8, False)])
@pytest.mark.parametrize("name", ["bf16", "f16_small", "f16_mixed", "f32"])
def test_unit_scale_and_statistic_is_quantize_search(name, bits, sym):
    from awq_quantizer import _hip
    dev = _dev()
    w = _search_case(name)
    R, K = w.shape
    gs = 128
    G = K // gs
    if name.startswith("f16"):
        sc = orc.quantize_groups(w, R, K, gs, bits, sym)[1].float()
        assert (sc < 14).all() if name == "f16_small" else ((sc >= 14).any() and (sc < 14).any())
    one = torch.ones(K)
    got = run_clip(w, one, one, gs, bits, sym)
    ref = {"qweight": torch.empty((R, K * bits // 32), dtype=torch.int32, device=dev),
           "qzeros": torch.empty((R, -(-G * bits // 32)), dtype=torch.int32, device=dev),
           "scales": torch.empty((R, G), dtype=torch.float16, device=dev)}
    _hip.quantize_search(w.to(dev), R, K, gs, bits, sym, GRID, CAND, **ref)
    for k in ("qweight", "qzeros"):
        assert torch.equal(got[k], ref[k].cpu()), k
    assert torch.equal(got["scales"].view(torch.int16), ref["scales"].cpu().view(torch.int16))
    if bits == 4:       # (at 8 bits no group of these inputs prefers a shrunk range without weights)
        assert got["best_idx"].any()


# ---------------------------------------------------------------- 4. identity (c)
@pytest.mark.parametrize("dtype,gs,bits,sym", [(torch.bfloat16, 128, 4, False), (torch.float16, 64, 4, True),
                                                (torch.float32, 256, 8, False), (torch.float16, 16, 4, False)])
def test_candidate_zero_loss_is_the_scale_search_partial(dtype, gs, bits, sym):
    from awq_quantizer import _hip
    dev = _dev()
    w, s, xs = weights((9, 1024), dtype, 5), col_scale(1024, 5), col_stat(1024, 5)
    got = run_clip(w, s, xs, gs, bits, sym)
    part = _hip.act_search_losses([w.to(dev)], xs.to(dev), s.to(dev).reshape(1, -1), gs, bits, sym).cpu().numpy()
    assert np.array_equal(got["loss"][0].view(np.int32), part[0].view(np.int32))


# ---------------------------------------------------------------- 5. the fallback kernel
def _raw_call(w_dev, s, xs, gs, bits, sym, rs=None, n_cand=CAND):
    """The C entry point on an arbitrary device pointer (w_dev: a possibly misaligned view)."""
    from awq_quantizer import _hip
    dev = w_dev.device
    R, K = w_dev.shape
    G = K // gs
    out = {"qweight": torch.full((R, K * bits // 32), -1, dtype=torch.int32, device=dev),
           "qzeros": torch.full((R, -(-G * bits // 32)), -1, dtype=torch.int32, device=dev),
           "scales": torch.full((R, G), -1.0, dtype=torch.float16, device=dev),
           "best_idx": torch.full((R * G,), -1, dtype=torch.int32, device=dev)}
    loss = torch.full((2, R * G), -1.0, dtype=torch.float32, device=dev)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = _hip.load_library().awq_quantize_clip_scaled(
        p(w_dev), _hip.AWQ_DTYPE[w_dev.dtype], R, K, gs, bits, int(sym), p(s), p(rs), p(xs), GRID, n_cand,
        p(out["qweight"]), p(out["qzeros"]), p(out["scales"]), p(out["best_idx"]), p(loss), R * G,
        ctypes.c_void_p(_hip.stream_ptr(dev)))
    assert rc == 0, _hip.last_error()
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in out.items()}
    got["loss"] = loss.cpu().numpy()
    return got


@pytest.mark.parametrize("gs,bits,sym", [(32, 4, False), (128, 4, True), (256, 8, False)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_misaligned_view_takes_the_fallback_with_the_same_bits(dtype, gs, bits, sym):
    dev = _dev()
    shape = (9, 3072)
    w, s, xs, want = grid_case(dtype, gs, bits, sym, shape)
    buf = torch.empty(w.numel() + 1, dtype=dtype, device=dev)
    view = buf[1:].view(shape)                     # element-aligned only
    view.copy_(w)
    assert view.data_ptr() % 16 != 0
    got = _raw_call(view, s.to(dev), xs.to(dev), gs, bits, sym)
    assert_same(got, want, "fallback vs expectation")
    assert_same(got, run_clip(w, s, xs, gs, bits, sym), "fallback vs streaming")


@pytest.mark.parametrize("bits,sym", [(4, False), (8, True)])
@pytest.mark.parametrize("gs,shape", [(8, (3, 64)), (16, (3, 64)), (8, (2, 1024)), (16, (2, 1024)), (512, (2, 1024))])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fallback_group_sizes(dtype, gs, bits, sym, shape):
    _dev()
    seed = gs + bits
    w, s, xs = weights(shape, dtype, seed), col_scale(shape[1], seed), col_stat(shape[1], seed)
    assert_same(run_clip(w, s, xs, gs, bits, sym), expect_clip(w, s, xs, gs, bits, sym, GRID, CAND))


# ---------------------------------------------------------------- 6. col_rscale paths
@pytest.mark.parametrize("dtype", DTYPES)
def test_reciprocal_table_paths_agree(dtype):
    from awq_quantizer import _hip
    dev = _dev()
    shape = (6, 1024)
    w, s, xs = weights(shape, dtype, 11), col_scale(shape[1], 11), col_stat(shape[1], 11)
    want = expect_clip(w, s, xs, 128, 4, False, GRID, CAND)
    assert_same(run_clip(w, s, xs, 128, 4, False, rscale="table"), want, "table")
    assert_same(run_clip(w, s, xs, 128, 4, False, rscale=None), want, "IEEE")
    # one column outside the Markstein quotient's proven range: its reciprocal is NaN, the wave
    # redoes the candidate with IEEE divisions
    s2 = s.clone()
    s2[130] = 2.0 ** -70
    rs = _hip.act_recip_table(s2.to(dev).reshape(1, -1)).reshape(-1)
    assert torch.isnan(rs[130]) and not torch.isnan(rs[131])
    want2 = expect_clip(w, s2, xs, 128, 4, False, GRID, CAND)
    a = run_clip(w, s2, xs, 128, 4, False, rscale=rs)
    b = run_clip(w, s2, xs, 128, 4, False, rscale=None)
    assert_same(a, want2, "table with a NaN entry")
    assert_same(b, want2, "IEEE")


# ---------------------------------------------------------------- 7. special values
@pytest.mark.parametrize("case", ["nan", "inf", "ninf", "constant", "xsq_nan"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_groups_keep_candidate_zero(dtype, case):
    """A NaN or +-inf weight, an all-equal group and a NaN statistic: the affected group keeps
    candidate 0 and its outputs are awq_quantize_groups_scaled's; every group matches the
    expectation."""
    from awq_quantizer import _hip
    dev = _dev()
    R, K, gs = 4, 512, 128
    w, s, xs = weights((R, K), dtype, 21), col_scale(K, 21), col_stat(K, 21)
    r, g = 2, 1                                     # the affected group
    if case == "nan":
        w[r, g * gs + 5] = float("nan")
    elif case == "inf":
        w[r, g * gs + 5] = float("inf")
    elif case == "ninf":
        w[r, g * gs + 5] = float("-inf")
    elif case == "constant":
        w[r, g * gs:(g + 1) * gs] = 0.0             # scale 0 for fp16, the 1e-10 clamp otherwise
    else:
        xs[g * gs + 7] = float("nan")
    got = run_clip(w, s, xs, gs, 4, False)
    assert_same(got, expect_clip(w, s, xs, gs, 4, False, GRID, CAND))
    G = K // gs
    rows = range(R) if case == "xsq_nan" else [r]
    ref = {"qweight": torch.empty((R, K // 8), dtype=torch.int32, device=dev),
           "qzeros": torch.empty((R, 1), dtype=torch.int32, device=dev),
           "scales": torch.empty((R, G), dtype=torch.float16, device=dev)}
    _hip.quantize_groups_scaled(w.to(dev), s.to(dev), gs, 4, False, **ref)
    for rr in rows:
        assert got["best_idx"][rr * G + g] == 0
        words = slice(g * gs // 8, (g + 1) * gs // 8)
        assert torch.equal(got["qweight"][rr, words], ref["qweight"].cpu()[rr, words])
        assert got["scales"].view(torch.int16)[rr, g] == ref["scales"].cpu().view(torch.int16)[rr, g]
        assert (got["qzeros"][rr, 0] >> (4 * g)) & 15 == (ref["qzeros"].cpu()[rr, 0] >> (4 * g)) & 15
    assert got["best_idx"].any()                    # the other groups still search


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_statistic_entry(dtype):
    """x_sq[k] = 0 removes column k from the loss (its error is free); the winner follows the
    definition, so the comparison is against the expectation."""
    _dev()
    w, s, xs = weights((4, 512), dtype, 22), col_scale(512, 22), col_stat(512, 22)
    xs[128 + 7] = 0.0
    assert_same(run_clip(w, s, xs, 128, 4, False), expect_clip(w, s, xs, 128, 4, False, GRID, CAND))


# ---------------------------------------------------------------- 8. quantize_layer_group(clip=True)
def _layer_quantizer(bits, gs, sym, duo, grid=8):
    from awq_quantizer.quantization import AWQQuantizer
    return AWQQuantizer(bits=bits, group_size=gs, symmetric=sym, scale_method="awq", search_grid=grid, duo_scaling=duo,
                        device="cuda:0", logger_level="ERROR")


@pytest.mark.parametrize("duo", [True, False])
@pytest.mark.parametrize("dtype,sym", [(torch.bfloat16, False), (torch.float16, True)])
def test_layer_group_clip_end_to_end(dtype, sym, duo):
    from awq_quantizer import _hip
    dev = _dev()
    K, gs = 1024, 128
    ws = {"q": weights((24, K), dtype, 31), "k": weights((8, K), dtype, 32), "v": weights((5, K), dtype, 33)}
    g = torch.Generator().manual_seed(34)
    x = (torch.randn(96, K, generator=g) * (1 + 10 * (torch.rand(K, generator=g) < 0.05))).to(dtype)
    q = _layer_quantizer(4, gs, sym, duo)
    plain = q.quantize_layer_group(ws, x)
    out = q.quantize_layer_group(ws, x, clip=True, clip_grid=GRID, clip_max_shrink=0.5)
    s = out["input_scale"]
    assert torch.equal(s, plain["input_scale"]) and out["best"] == plain["best"]
    xs = _hip.act_stats(x.to(dev))[1]
    clipped = total = 0
    for name, w in ws.items():
        # clip=False is unchanged: awq_quantize_groups_scaled's bits
        R = w.shape[0]
        ref = {"qweight": torch.empty((R, K // 8), dtype=torch.int32, device=dev),
               "qzeros": torch.empty((R, 1), dtype=torch.int32, device=dev),
               "scales": torch.empty((R, K // gs), dtype=torch.float16, device=dev)}
        _hip.quantize_groups_scaled(w.to(dev), s, gs, 4, sym, **ref)
        for k in ref:
            assert torch.equal(plain["results"][name][k].view(torch.int32 if k != "scales" else torch.int16),
                               ref[k].view(torch.int32 if k != "scales" else torch.int16)), (name, k)
        # clip=True equals the raw call
        raw = run_clip(w, s.cpu(), xs.cpu(), gs, 4, sym, GRID, CAND)
        r = out["results"][name]
        assert sorted(r) == sorted(plain["results"][name])
        assert torch.equal(r["qweight"].cpu(), raw["qweight"]) and torch.equal(r["qzeros"].cpu(), raw["qzeros"])
        assert torch.equal(r["scales"].cpu().view(torch.int16), raw["scales"].view(torch.int16))
        assert torch.equal(r["input_scale"], s)
        nz = int((raw["best_idx"] != 0).sum())
        assert out["clip"]["per_weight"][name]["clipped_fraction"] == nz / raw["best_idx"].numel()
        clipped += nz
        total += raw["best_idx"].numel()
    c = out["clip"]
    assert c["clipped_fraction"] == clipped / total and clipped > 0
    assert c["loss_after"] <= c["loss_before"]
    # the three linears' candidate-0 losses in one buffer: the scale search's loss of its winner
    assert np.float64(c["loss_before"]).view(np.int64) == plain["losses"].cpu().numpy()[plain["best"]].view(np.int64)


# ---------------------------------------------------------------- 9. the CLI
def test_cli_act_clip_equals_the_api(tmp_path):
    from safetensors.torch import save_file
    from awq_quantizer.main import main
    _dev()
    K = 512
    ws = {"a.weight": weights((16, K), torch.bfloat16, 41), "b.weight": weights((8, K), torch.bfloat16, 42)}
    src = tmp_path / "model"
    src.mkdir()
    save_file(ws, str(src / "model.safetensors"))
    g = torch.Generator().manual_seed(43)
    stats = {}
    for name in ws:
        x = torch.randn(64, K, generator=g) * (1 + 10 * (torch.rand(K, generator=g) < 0.05))
        stats[name] = (x.abs().mean(0).float(), (x * x).mean(0).float())
    sfile = str(tmp_path / "stats.safetensors")
    save_file({f"{n}.{k}": v for n, (xm, xq) in stats.items() for k, v in (("x_mean", xm), ("x_sq", xq))}, sfile)
    out = tmp_path / "out"
    assert main(["--model_id", str(src), "--output_dir", str(out), "--scale_method", "awq", "--act_stats", sfile,
                 "--act_clip", "--clip_grid", "20", "--clip_max_shrink", "0.5", "--output_format", "packed",
                 "--log_level", "ERROR"]) == 0
    meta = json.load(open(out / "metadata.json"))
    q = _layer_quantizer(4, 128, False, True, grid=20)
    for name, w in ws.items():
        res = torch.load(str(out / f"model_chunk_{meta['tensor_to_chunk'][name]:04d}.pt"), weights_only=True)[name]
        xm, xq = stats[name]
        api = q.quantize_layer_group({name: w}, x_mean=xm, x_sq=xq, clip=True, clip_grid=20, clip_max_shrink=0.5)
        r = api["results"][name]
        assert api["clip"]["clipped_fraction"] > 0
        for k in ("qweight", "qzeros", "input_scale"):
            assert torch.equal(res[k], r[k].cpu()), (name, k)
        assert torch.equal(res["scales"].view(torch.int16), r["scales"].cpu().view(torch.int16)), name
