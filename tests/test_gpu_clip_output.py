"""Clip search with the token-sample loss on the GPU (include/awq_hip.h awq_quantize_clip_output;
DESIGN.md §5.14): both kernels against float64 losses put together in numpy from the test's own
reader of the packed layout, and the Python API on top of them.

  * a forced candidate 0 is RTN of W diag(s), bit for bit;
  * exact data — every product and partial sum is exact in fp32 in any order: the loss of
    candidate 0 equals the float64 one within the fp32 sum over the tokens;
  * random data — the header's accuracy contract for every candidate's loss;
  * the selection, checked exactly on the returned values, and the packed bits of the winners;
  * non-finite inputs, determinism, guard bands, the capped grid's later trips, the API.

The parts are functions part_*; test_clip_output at the end of the file runs them all, and the
model-level part of test_gpu_clip_output_model.py, under one test id."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_gpu_bounds import Call, elem_mask

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
I32 = torch.int32
_ids = lambda v: str(v).replace("torch.", "")
GRIDS = [(20, 10), (4, 4)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from awq_quantizer import _hip
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    return dev


def eps_l(L, f32_operands):
    return (0.0 if f32_operands else 2.0 ** -17) + L * 2.0 ** -22


def each(fn, cases):
    """fn(dev, *case) for every case of one test, the case named in the failure it raises"""
    dev = _dev()
    for c in cases:
        try:
            fn(dev, *c)
        except AssertionError as e:
            raise AssertionError(f"case {_ids(c)}: {e}") from e


# ---------------------------------------------------------------- the test's own reader (numpy)
def unpack_fields(words: np.ndarray, bits: int, n: int) -> np.ndarray:
    per = 32 // bits
    w = words.view(np.uint32).astype(np.int64)
    out = np.stack([(w >> (j * bits)) & ((1 << bits) - 1) for j in range(per)], axis=-1)
    return out.reshape(w.shape[0], -1)[:, :n]


def dequant_np(qweight, qzeros, scales, bits, gs, K) -> np.ndarray:
    """fp32(fp16(fp16(q - z) * s)) [N, K] from the packed row-major layout."""
    q = unpack_fields(qweight, bits, K)
    z = unpack_fields(qzeros, bits, K // gs)
    diff = (q - np.repeat(z, gs, axis=1)).astype(np.float16)
    s = np.repeat(scales.view(np.float16), gs, axis=1)
    with np.errstate(all="ignore"):
        return (diff * s).astype(np.float16).astype(np.float32)


def d_of(w32, dq, col):
    """d = RN_f32(RN_f32(dq / col_scale) - w)"""
    with np.errstate(all="ignore"):
        return ((dq / col[None, :].astype(np.float32)).astype(np.float32) - w32).astype(np.float32)


def to_np32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().float().numpy()


def group_products(d64, x64, gs):
    """E* [N, G, T] = sum over the group's k of d x, and A = the same of |d| |x| (float64)"""
    N, K = d64.shape
    G = K // gs
    dg = d64.reshape(N, G, gs)
    xg = x64.reshape(x64.shape[0], G, gs)
    return np.einsum("ngk,tgk->ngt", dg, xg), np.einsum("ngk,tgk->ngt", np.abs(dg), np.abs(xg))


def loss_and_bound(E, A, eps, T):
    """L* = sum_t E*^2 and the contract's bound on a returned loss: sum_t (2 |E*| delta + delta^2)
    + (T + 2) 2^-24 (L* + that), delta = eps A"""
    L = (E ** 2).sum(axis=2)
    delta = eps * A
    b = (2 * np.abs(E) * delta + delta ** 2).sum(axis=2)
    return L, b + (T + 2) * 2.0 ** -24 * (L + b)


# ---------------------------------------------------------------- running the entry
def strided(x: torch.Tensor, pad: int, dev) -> torch.Tensor:
    T, K = x.shape
    buf = torch.full((T, K + pad), 7.0, dtype=x.dtype, device=dev)
    buf[:, :K] = x.to(dev)
    return buf[:, :K]


def skewed(t: torch.Tensor, dev) -> torch.Tensor:
    """a contiguous device copy that starts one element past a 256-B boundary"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


def is_fast(case):
    return case["w"].dtype == BF16 and case["gs"] in (32, 64, 128, 256) and not case["skew"] and case["pad"] % 8 == 0


def make_case(w, x, s, gs, bits, sym, pad=0, skew=False):
    return {"w": w, "x": x, "s": np.ascontiguousarray(s, dtype=np.float32), "gs": gs, "bits": bits, "sym": sym,
            "pad": pad, "skew": skew}


JUNK = 0x5A


def run(dev, case, n_grid, c0, nc, *, rscale=True, outs=("qweight", "qzeros", "scales", "best_idx", "group_loss", "cand_loss")):
    """One call; every requested output starts from junk bytes.  -> dict of numpy arrays.
    rscale: True the reciprocal table, False NULL (IEEE divisions from the start), "nan" the table
    with every fifth entry NaN (the candidates are redone with IEEE divisions): the same bits.
    The entry's own predicate must send the case to the kernel the test means to reach."""
    from awq_quantizer import _hip
    w = skewed(case["w"], dev) if case["skew"] else case["w"].to(dev)
    x = skewed(case["x"], dev) if case["skew"] else (strided(case["x"], case["pad"], dev) if case["pad"] else case["x"].to(dev))
    s = torch.from_numpy(case["s"]).to(dev)
    rs = _hip.act_recip_table(s.reshape(1, -1)).reshape(-1) if rscale else None
    if rscale == "nan":
        rs[::5] = float("nan")
    N, K = w.shape
    gs, bits = case["gs"], case["bits"]
    G, per = K // gs, 32 // bits
    shapes = {"qweight": ((N, K // per), I32), "qzeros": ((N, -(-G // per)), I32), "scales": ((N, G), F16),
              "best_idx": ((N * G,), I32), "group_loss": ((2, N * G), F32), "cand_loss": ((nc, N * G), F32)}
    bufs = {}
    for k in outs:
        shape, dt = shapes[k]
        bufs[k] = torch.empty(shape, dtype=dt, device=dev)
        bufs[k].view(-1).view(torch.uint8).fill_(JUNK)
    assert _hip.clip_output_fast(w, s, x, gs, rs) == is_fast(case), "the entry routes this case to the other kernel"
    _hip.quantize_clip_output(w, s, x, gs, bits, case["sym"], n_grid, nc, cand_begin=c0, rscale=rs, **bufs)
    torch.cuda.synchronize(dev)
    out = {k: v.cpu() for k, v in bufs.items()}
    if "scales" in out:
        out["scales"] = out["scales"].view(torch.int16)
    return {k: v.numpy() for k, v in out.items()}


def rtn_scaled(dev, case):
    """RTN of W diag(s): awq_quantize_groups_scaled where it takes the shape, else the two calls it
    is defined by (awq_apply_input_scale, then quantize_packed)."""
    from awq_quantizer import _hip
    from awq_quantizer.quantization import AWQQuantizer
    q = AWQQuantizer(bits=case["bits"], group_size=case["gs"], symmetric=case["sym"], device="cuda:0", logger_level="ERROR")
    w = case["w"].to(dev)
    s = torch.from_numpy(case["s"]).to(dev)
    if _hip.scaled_eligible(w.dtype, w.shape[0], w.shape[1], case["gs"]):
        r = q._packed_outputs(w)
        _hip.quantize_groups_scaled(w, s, case["gs"], case["bits"], case["sym"], qweight=r["qweight"], qzeros=r["qzeros"],
                                    scales=r["scales"])
    else:
        r = q.quantize_packed(_hip.apply_input_scale(w, s))
    torch.cuda.synchronize(dev)
    return {"qweight": r["qweight"].cpu().numpy(), "qzeros": r["qzeros"].cpu().numpy(),
            "scales": r["scales"].cpu().view(torch.int16).numpy()}


def d64_of(case, packed):
    K = case["w"].shape[1]
    dq = dequant_np(packed["qweight"], packed["qzeros"], packed["scales"].view(np.uint16), case["bits"], case["gs"], K)
    return d_of(to_np32(case["w"]), dq, case["s"]).astype(np.float64)


def group_bits(case, packed):
    """(weight words [N, G, words per group], zero fields [N, G], scale bits [N, G])"""
    N, K = case["w"].shape
    gs, bits = case["gs"], case["bits"]
    G = K // gs
    return (packed["qweight"].reshape(N, G, -1), unpack_fields(packed["qzeros"], bits, G), packed["scales"].view(np.uint16))


# ---------------------------------------------------------------- inputs
def random_case(N, K, T, gs, bits, sym, dtype, seed, pad=0, skew=False):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.02).to(dtype)
    x = torch.randn(T, K, generator=g).to(dtype)
    s = torch.exp((torch.rand(K, generator=g) * 2 - 1) * math.log(4.0)).numpy()
    return make_case(w, x, s, gs, bits, sym, pad, skew)


def exact_case(N, K, T, gs, sym, dtype, seed, pad=0, skew=False):
    """4-bit.  w = m 2^-8, |m| <= 240; s powers of two in [1/2, 2], s = 2 at one column of every
    group, where every row holds |m| = 240 (and 0 at another column): the range of w' is 480 / 256
    (symmetric: +-480 / 256), so RTN's scale is 2^-3 (2^-2) and z = 0 (none); x integers in
    [-2, 2].  d then lies on the 2^-8 grid and every partial sum of d x fits fp32 in any order."""
    rng = np.random.default_rng(seed)
    G = K // gs
    m = rng.integers(0, 241, size=(N, K))
    if sym:
        m = m * rng.choice([-1, 1], size=(N, K))
    s = 2.0 ** rng.integers(-1, 2, size=K)
    for g in range(G):
        p_max, p_zero = g * gs + (3 * g + 1) % gs, g * gs + (3 * g + 5) % gs
        s[p_max] = 2.0
        m[:, p_max] = 240 if not sym else 240 * rng.choice([-1, 1], size=N)
        m[:, p_zero] = 0
    w = torch.from_numpy((m / 256.0).astype(np.float32)).to(dtype)
    assert np.array_equal(to_np32(w), (m / 256.0).astype(np.float32))
    x = torch.from_numpy(rng.integers(-2, 3, size=(T, K)).astype(np.float32)).to(dtype)
    return make_case(w, x, s, gs, 4, sym, pad, skew)


# rows x K x T: G = 1, G % 8 != 0, more than one qzeros word; token-tile edges, a partial tile, more
# than one LDS chunk (128 tokens; 64 at group_size 256: T = 65)
def fast_cases():
    out = []
    shapes = [(1, 1, 1), (33, 3, 33), (130, 9, 129), (33, 3, 300), (130, 1, 65)]
    for i, gs in enumerate((32, 64, 128, 256)):
        for j, (N, ng, T) in enumerate(shapes):
            v = i + j
            out.append((N, ng * gs, T, gs, 8 if v % 3 == 2 else 4, bool(v & 1), BF16, 8 * ((v >> 1) & 1), False))
    return out


def generic_cases():
    return [(33, 3 * 8, 33, 8, 4, False, BF16, 0, False), (130, 9 * 16, 129, 16, 8, True, BF16, 3, False),
            (33, 3 * 512, 65, 512, 4, True, BF16, 0, False), (1, 512, 1, 512, 8, False, F32, 0, False),
            (33, 3 * 32, 300, 32, 4, False, F16, 3, False), (130, 9 * 64, 33, 64, 8, True, F32, 0, False),
            (33, 3 * 128, 129, 128, 4, True, F16, 0, False), (130, 256, 65, 256, 4, False, F32, 3, False),
            (33, 3 * 64, 129, 64, 4, False, BF16, 0, True), (130, 9 * 32, 33, 32, 8, True, BF16, 0, True),
            (33, 3 * 128, 300, 128, 4, False, BF16, 3, False)]


# ---------------------------------------------------------------- 1. forced candidate 0 is RTN
def _forced_zero(dev, N, K, T, gs, bits, sym, dtype, pad, skew):
    case = random_case(N, K, T, gs, bits, sym, dtype, seed=N + K + T + bits, pad=pad, skew=skew)
    for n_grid in (20, 4):
        got = run(dev, case, n_grid, 0, 1)
        want = rtn_scaled(dev, case)
        for k in ("qweight", "qzeros", "scales"):
            assert np.array_equal(got[k], want[k]), k
        assert np.all(got["best_idx"] == 0)
        assert np.array_equal(got["group_loss"][0].view(np.int32), got["cand_loss"][0].view(np.int32))
        assert np.array_equal(got["group_loss"][1].view(np.int32), got["cand_loss"][0].view(np.int32))


def part_forced_candidate_zero_is_rtn_fast():
    cases = fast_cases()
    assert all(is_fast(make_case(torch.empty(0, dtype=c[6]), None, [], c[3], c[4], c[5], c[7], c[8])) for c in cases)
    each(_forced_zero, cases)


def part_forced_candidate_zero_is_rtn_generic():
    cases = generic_cases()
    assert not any(is_fast(make_case(torch.empty(0, dtype=c[6]), None, [], c[3], c[4], c[5], c[7], c[8])) for c in cases)
    each(_forced_zero, cases)


# ---------------------------------------------------------------- 2. exact data, candidate 0
def _exact(dev, N, K, T, gs, sym, dtype, pad, skew):
    from awq_quantizer import _hip
    case = exact_case(N, K, T, gs, sym, dtype, seed=N + K + T, pad=pad, skew=skew)
    got = run(dev, case, 20, 0, 1)
    G = K // gs
    scale = got["scales"].view(np.float16).astype(np.float64)
    assert np.all(scale == (0.25 if sym else 0.125)), "the construction's RTN scale"
    d64 = d64_of(case, got)
    x64 = to_np32(case["x"]).astype(np.float64)
    E, A = group_products(d64, x64, gs)
    assert np.array_equal(d64 * 256, np.round(d64 * 256)) and A.max() * 256 < 2 ** 24
    assert (d64 != 0).mean() > 0.5
    want = (E ** 2).sum(axis=2).reshape(-1)
    loss = got["cand_loss"][0].astype(np.float64)
    tol = (T + 2) * 2.0 ** -24
    assert np.all(np.abs(loss - want) <= tol * want), float(np.abs(loss / np.maximum(want, 1e-300) - 1).max())
    if G == 1:        # the same sums from awq_output_error on the RTN result
        e_sq, _, _ = _hip.output_error(case["w"].to(dev), gs, 4, sym, torch.from_numpy(got["qweight"]).to(dev),
                                       torch.from_numpy(got["qzeros"]).to(dev),
                                       torch.from_numpy(got["scales"]).to(dev).view(F16), case["x"].to(dev),
                                       torch.from_numpy(case["s"]).to(dev), ref=False)
        assert np.all(np.abs(e_sq.cpu().numpy().astype(np.float64) - loss) <= 2 * tol * want)


EXACT_FAST = [(N, K, T, gs, sym, BF16, pad, False) for (N, K, T, gs, _b, sym, _d, pad, _s) in fast_cases()]
EXACT_GENERIC = [(N, K, T, gs, sym, dt, pad, skew) for (N, K, T, gs, _b, sym, dt, pad, skew) in generic_cases()]


def part_exact_fast():
    each(_exact, EXACT_FAST)


def part_exact_generic():
    each(_exact, EXACT_GENERIC)


# ---------------------------------------------------------------- 3. / 4. random data: contract and selection
_RUNS = {}


def runs_of(dev, key, n_grid, nc):
    """The full run and the forced run of every candidate of one random case, computed once."""
    k = (key, n_grid, nc)
    if k not in _RUNS:
        N, K, T, gs, bits, sym, dtype, pad, skew = key
        case = random_case(N, K, T, gs, bits, sym, dtype, seed=N + K + T + bits + 1, pad=pad, skew=skew)
        full = run(dev, case, n_grid, 0, nc)
        forced = [run(dev, case, n_grid, i, 1) for i in range(nc)]
        x64 = to_np32(case["x"]).astype(np.float64)
        eps = eps_l(gs, not is_fast(case))
        LB = [loss_and_bound(*group_products(d64_of(case, f), x64, gs), eps, T) for f in forced]
        _RUNS[k] = (case, full, forced, np.stack([l for l, _ in LB]).reshape(nc, -1), np.stack([b for _, b in LB]).reshape(nc, -1))
    return _RUNS[k]


RANDOM_FAST = [(33, 3 * 32, 33, 32, 4, False, BF16, 8, False), (130, 9 * 64, 129, 64, 8, True, BF16, 0, False),
               (33, 3 * 128, 300, 128, 4, True, BF16, 0, False), (130, 256, 65, 256, 4, False, BF16, 8, False),
               (1, 128, 1, 128, 8, False, BF16, 0, False)]
RANDOM_GENERIC = [(33, 3 * 8, 33, 8, 4, False, BF16, 0, False), (33, 3 * 16, 129, 16, 8, True, F16, 3, False),
                  (33, 1024, 65, 512, 4, True, F32, 0, False), (130, 9 * 32, 33, 32, 4, False, F32, 3, False),
                  (33, 3 * 64, 300, 64, 4, False, BF16, 0, True)]


def _contract(dev, *key):
    worst = 0.0
    for n_grid, nc in GRIDS:
        case, full, forced, L, B = runs_of(dev, key, n_grid, nc)
        T = key[2]
        for i in range(nc):
            loss = full["cand_loss"][i].astype(np.float64)
            assert np.array_equal(full["cand_loss"][i].view(np.int32), forced[i]["cand_loss"][0].view(np.int32)), \
                f"candidate {i}: the forced run's loss differs"
            assert np.all(np.abs(loss - L[i]) <= B[i]), f"candidate {i} of {n_grid}"
            worst = max(worst, float((np.abs(loss - L[i]) / B[i]).max()))
    print(f"clip_output {_ids(key)}: the losses use at most {worst:.3e} of the contract's bound")


def part_random_contract_fast():
    each(_contract, RANDOM_FAST)


def part_random_contract_generic():
    each(_contract, RANDOM_GENERIC)


def _selection(dev, *key):
    from awq_quantizer import _hip
    for n_grid, nc in GRIDS:
        case, full, forced, L, B = runs_of(dev, key, n_grid, nc)
        cl, best = full["cand_loss"], full["best_idx"]
        # without the reciprocal table, and with NaN entries in it: the IEEE divisions give the same bytes
        for how in (False, "nan"):
            alt = run(dev, case, n_grid, 0, nc, rscale=how)
            for k in full:
                assert np.array_equal(alt[k].view(np.uint8), full[k].view(np.uint8)), f"rscale={how}: {k}"
        n = cl.shape[1]
        want = np.zeros(n, dtype=np.int32)
        lo = np.full(n, np.inf, dtype=np.float32)
        for i in range(nc):                       # the first strict minimum; a NaN never wins
            take = cl[i] < lo
            want[take], lo[take] = i, cl[i][take]
        assert np.array_equal(best, want)
        cols = np.arange(n)
        assert np.array_equal(full["group_loss"][0].view(np.int32), cl[0].view(np.int32))
        assert np.array_equal(full["group_loss"][1].view(np.int32), cl[best, cols].view(np.int32))
        # (sanity of the case, where it has groups enough; 8-bit fields and quarter steps rarely gain from a shrink)
        if n > 1 and case["bits"] == 4 and n_grid == 20:
            assert len(set(best.tolist())) > 1, "the case exercises one candidate only"
        # every group's packed bits are the forced run's for its winner
        N, K = case["w"].shape
        G = K // case["gs"]
        got = group_bits(case, full)
        b2 = best.reshape(N, G)
        for i in range(nc):
            ref = group_bits(case, forced[i])
            m = b2 == i
            for a, b, what in zip(got, ref, ("weight words", "zero field", "scale")):
                assert np.array_equal(a[m], b[m]), f"candidate {i}: {what}"
        # awq_quantize_clip_scaled's bits wherever it chose the same candidate
        w, s = case["w"].to(dev), torch.from_numpy(case["s"]).to(dev)
        x_sq = (case["x"].float() ** 2).mean(dim=0).to(dev)
        per = 32 // case["bits"]
        r = {"qweight": torch.empty((N, K // per), dtype=I32, device=dev),
             "qzeros": torch.empty((N, -(-G // per)), dtype=I32, device=dev),
             "scales": torch.empty((N, G), dtype=F16, device=dev)}
        idx = torch.empty(N * G, dtype=I32, device=dev)
        _hip.quantize_clip_scaled(w, s, x_sq, case["gs"], case["bits"], case["sym"], n_grid, nc, best_idx=idx, **r)
        diag = group_bits(case, {"qweight": r["qweight"].cpu().numpy(), "qzeros": r["qzeros"].cpu().numpy(),
                                 "scales": r["scales"].cpu().view(torch.int16).numpy()})
        same = idx.cpu().numpy().reshape(N, G) == b2
        assert same.any() or n == 1
        for a, b, what in zip(got, diag, ("weight words", "zero field", "scale")):
            assert np.array_equal(a[same], b[same]), f"awq_quantize_clip_scaled: {what}"
        # optimal against float64 within the two candidates' bounds
        imin = L.argmin(axis=0)
        assert np.all(L[best, cols] <= L[imin, cols] + B[best, cols] + B[imin, cols])


def part_selection_fast():
    each(_selection, RANDOM_FAST)


def part_selection_generic():
    each(_selection, RANDOM_GENERIC)


# ---------------------------------------------------------------- 5. non-finite
def _non_finite(dev, *key):
    N, K, T, gs, bits, sym, dtype, pad, skew = key
    G = K // gs
    case = random_case(N, K, T, gs, bits, sym, dtype, seed=5, pad=pad, skew=skew)
    clean = run(dev, case, 20, 0, 10)
    bad = dict(case, w=case["w"].clone())
    r0, g0 = min(5, N - 1), G - 1
    bad["w"][r0, g0 * gs + 3] = float("nan")
    got = run(dev, bad, 20, 0, 10)
    rtn = rtn_scaled(dev, bad)
    keep = np.ones((N, G), dtype=bool)
    keep[r0, g0] = False
    for a, b in zip(group_bits(bad, got), group_bits(case, clean)):
        assert np.array_equal(a[keep], b[keep])
    for a, b, what in zip(group_bits(bad, got), group_bits(bad, rtn), ("weight words", "zero field", "scale")):
        assert np.array_equal(a[~keep], b[~keep]), what
    assert np.isnan(got["scales"].view(np.float16).reshape(N, G)[r0, g0])
    flat = keep.reshape(-1)
    assert got["best_idx"][~flat] == 0 and np.array_equal(got["best_idx"][flat], clean["best_idx"][flat])
    for k in ("group_loss", "cand_loss"):
        assert np.array_equal(got[k][:, flat].view(np.int32), clean[k][:, flat].view(np.int32))
        assert not np.isfinite(got[k][:, ~flat]).any()
    inf = dict(case, x=case["x"].clone())
    inf["x"][min(3, T - 1), 1::gs] = float("inf")          # one sample of every group
    got = run(dev, inf, 20, 0, 10)
    rtn = rtn_scaled(dev, inf)
    assert not np.isfinite(got["cand_loss"]).any() and not np.isfinite(got["group_loss"]).any()
    assert np.all(got["best_idx"] == 0)
    for k in ("qweight", "qzeros", "scales"):
        assert np.array_equal(got[k], rtn[k]), k


def part_non_finite():
    each(_non_finite, [RANDOM_FAST[0], RANDOM_FAST[2], RANDOM_GENERIC[1], RANDOM_GENERIC[4]])


def part_no_tokens():
    """T = 0: every loss +0, every winner the first candidate, the packed outputs RTN's."""
    def one(dev, dtype, gs):
        case = random_case(33, 3 * gs, 1, gs, 4, False, dtype, seed=9)
        case["x"] = case["x"][:0]
        got = run(dev, case, 20, 0, 10)
        rtn = rtn_scaled(dev, case)
        assert np.all(got["cand_loss"].view(np.int32) == 0) and np.all(got["group_loss"].view(np.int32) == 0)
        assert np.all(got["best_idx"] == 0)
        for k in ("qweight", "qzeros", "scales"):
            assert np.array_equal(got[k], rtn[k]), k

    each(one, [(BF16, 64), (F32, 16)])


# ---------------------------------------------------------------- 6. determinism and guard bands
def part_deterministic():
    def one(dev, *key):
        case = random_case(*key[:7], seed=3, pad=key[7], skew=key[8])
        a, b = run(dev, case, 20, 0, 10), run(dev, case, 20, 0, 10)
        for k in a:
            assert np.array_equal(a[k].view(np.uint8) if a[k].dtype != np.float32 else a[k].view(np.int32),
                                  b[k].view(np.uint8) if b[k].dtype != np.float32 else b[k].view(np.int32)), k

    each(one, [RANDOM_FAST[2], RANDOM_GENERIC[4]])


OUTS = [("qweight", "qzeros", "scales", "best_idx", "group_loss", "cand_loss"), ("best_idx",), ("qzeros", "cand_loss"),
        ("qweight", "scales", "group_loss")]


def _arena_call(dev, case, n_grid, nc, outs, slack, want):
    """The call's buffers in a guard-band arena; -> (Call, launch)."""
    from awq_quantizer import _hip
    N, K = case["w"].shape
    gs, bits = case["gs"], case["bits"]
    n = N * (K // gs)
    stride = n + slack
    skew = case["w"].element_size() if case["skew"] else 0
    c = Call(dev, seed=K + bits + len(outs))
    wb = c.inp("w", case["w"], skew=skew, align=16)
    xb = c.inp("x", case["x"], skew=skew, align=16)
    sb = c.inp("col_scale", case["s"])
    rb = c.inp("col_rscale", _hip.act_recip_table(torch.from_numpy(case["s"]).to(dev).reshape(1, -1)).cpu())
    ob = {}
    for k in outs:
        if k in ("group_loss", "cand_loss"):
            rows = want[k].shape[0]
            full = np.zeros((rows, stride), dtype=np.float32)
            full[:, :n] = want[k]
            owned = torch.zeros((rows, stride), dtype=torch.bool)
            owned[:, :n] = True
            ob[k] = c.out(k, full, nan_dtype=F32, written=elem_mask(owned, 4))
        else:
            ob[k] = c.out(k, want[k])
    c.build()
    assert (wb.addr % 16 == 0 and xb.addr % 16 == 0) == (not case["skew"])
    p = lambda k: ob[k].ptr if k in ob else None
    T = case["x"].shape[0]
    launch = lambda: _hip.load_library().awq_quantize_clip_output(        # (the library of the moment: _hip.tuning)
        wb.ptr, _hip.AWQ_DTYPE[case["w"].dtype], N, K, gs, bits, int(case["sym"]), sb.ptr, rb.ptr, xb.ptr, T, K, n_grid, 0,
        nc, p("qweight"), p("qzeros"), p("scales"), p("best_idx"), p("group_loss"), p("cand_loss"), stride, None,
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return c, launch


def _guard_bands(dev, dtype, gs, bits, skew, outs, slack):
    N, K, T = 130, 3 * gs, 129
    assert (K // gs) % (32 // bits) != 0                     # qzeros words with unused fields
    case = random_case(N, K, T, gs, bits, False, dtype, seed=7, skew=skew)
    want = run(dev, case, 20, 0, 10)
    c, launch = _arena_call(dev, case, 20, 10, outs, slack, want)
    c.run(launch)


def part_guard_bands():
    """Every buffer out of a guard-band arena, both fills, every optional output on and off: the
    outputs are fully written (qzeros too, where its words hold unused fields), nothing else is."""
    cases = [(BF16, 64, 4, False, o, 37 * (i & 1)) for i, o in enumerate(OUTS)]
    cases += [(BF16, 64, 8, True, o, 0) for o in OUTS] + [(F32, 16, 4, False, OUTS[0], 5)]
    each(_guard_bands, cases)


# ---------------------------------------------------------------- 7. later loop trips
def part_capped_grid_later_trips():
    """max_blocks = 2: the fast kernel's 6 tiles ((130 rows -> 2 row blocks) x 3 groups) take three
    trips, the generic kernel's 390 groups many; every capped call reproduces the uncapped bytes."""
    def one(dev, dtype, gs, skew):
        from awq_quantizer import _hip
        case = random_case(130, 3 * gs, 33, gs, 4, False, dtype, seed=13, skew=skew)
        want = run(dev, case, 20, 0, 10)
        c, launch = _arena_call(dev, case, 20, 10, OUTS[0], 0, want)
        c.run(launch)
        base = {b.name: b.region.u8.cpu().clone() for b in c.bufs if b.expect is not None}
        with _hip.tuning(max_blocks=2):
            c.run(launch)
        for b in c.bufs:
            if b.expect is not None:
                assert torch.equal(b.region.u8.cpu(), base[b.name]), b.name

    each(one, [(BF16, 64, False), (BF16, 64, True), (F16, 16, False)])


# ---------------------------------------------------------------- 8. the Python API
def _quantizer(**kw):
    from awq_quantizer.quantization import AWQQuantizer
    return AWQQuantizer(**dict(dict(bits=4, group_size=32, symmetric=False, device="cuda:0", logger_level="ERROR",
                                    scale_method="awq", search_grid=8), **kw))


def _api_inputs():
    g = torch.Generator().manual_seed(31)
    ws = {"a": (torch.randn(64, 128, generator=g) * 0.02).to(BF16), "b": (torch.randn(96, 128, generator=g) * 0.02).to(BF16)}
    x = (torch.randn(48, 128, generator=g) * (0.25 + 4 * torch.rand(128, generator=g) ** 3)).to(BF16)
    return ws, x


def part_api_clip_loss_output():
    dev = _dev()
    from awq_quantizer.quantization import act_search
    q = _quantizer()
    ws, x = _api_inputs()
    diag = q.quantize_layer_group(ws, x, clip=True)
    out = act_search.quantize_layer_group(q, ws, x, clip=True, clip_loss="output", samples=x)
    assert set(out) == set(diag) and set(out["clip"]) == set(diag["clip"]) | {"loss"}
    clip = out["clip"]
    assert clip["loss"] == "output" and "loss" not in diag["clip"]
    assert clip["loss_after"] <= clip["loss_before"] and 0 < clip["clipped_fraction"] <= 1
    assert set(clip["per_weight"]) == set(ws) and set(clip["best_idx"]) == set(ws)
    assert torch.equal(out["input_scale"], diag["input_scale"]) and out["best"] == diag["best"]
    # the results dequantize to the float64 losses reported
    s = out["input_scale"].cpu().numpy()
    x64 = to_np32(x).astype(np.float64)
    after, bound = 0.0, 0.0
    for name, w in ws.items():
        r = out["results"][name]
        assert torch.equal(r["input_scale"], out["input_scale"])
        wh = q.dequantize_packed({k: v for k, v in r.items() if k != "input_scale"}).cpu().numpy()
        d64 = d_of(to_np32(w), wh, s).astype(np.float64)
        L, B = loss_and_bound(*group_products(d64, x64, 32), eps_l(32, False), 48)
        per = clip["per_weight"][name]
        assert abs(per["loss_after"] - L.sum()) <= B.sum(), name
        assert per["loss_after"] <= per["loss_before"]
        after, bound = after + L.sum(), bound + B.sum()
    assert abs(clip["loss_after"] - after) <= bound
    # the quantizer's own setting reaches the methods (their signatures are the class's)
    q2 = _quantizer()
    q2.clip_loss = "output"
    again = q2.quantize_layer_group(ws, x, clip=True)
    assert again["clip"]["loss"] == "output"
    for name in ws:
        for k in ("qweight", "qzeros", "scales"):
            assert torch.equal(again["results"][name][k], out["results"][name][k])
    # composes with loss="output"
    both = act_search.quantize_layer_group(q, ws, x, clip=True, clip_loss="output", loss="output")
    assert both["loss"] == "output" and both["clip"]["loss"] == "output"
    assert both["clip"]["loss_after"] <= both["clip"]["loss_before"]


def part_api_clip_loss_diag_is_todays_call():
    dev = _dev()
    from awq_quantizer.quantization import act_search
    q = _quantizer()
    ws, x = _api_inputs()
    a = q.quantize_layer_group(ws, x, clip=True)
    b = act_search.quantize_layer_group(q, ws, x, clip=True, clip_loss="diag")
    assert set(a) == set(b) and a["clip"]["loss_before"] == b["clip"]["loss_before"]
    assert a["clip"]["loss_after"] == b["clip"]["loss_after"] and "loss" not in b["clip"]
    for name in ws:
        for k in ("qweight", "qzeros", "scales", "input_scale"):
            assert torch.equal(a["results"][name][k], b["results"][name][k])
        assert torch.equal(a["clip"]["best_idx"][name], b["clip"]["best_idx"][name])


# ---------------------------------------------------------------- the one test id
def _parts():
    from test_gpu_clip_output_model import part_checkpoint
    return [part_forced_candidate_zero_is_rtn_fast, part_forced_candidate_zero_is_rtn_generic, part_exact_fast,
            part_exact_generic, part_random_contract_fast, part_random_contract_generic, part_selection_fast,
            part_selection_generic, part_non_finite, part_no_tokens, part_deterministic, part_guard_bands,
            part_capped_grid_later_trips, part_api_clip_loss_output, part_api_clip_loss_diag_is_todays_call,
            part_checkpoint]


def test_clip_output(tmp_path):
    """Every part above, and the model-level part of test_gpu_clip_output_model.py, under one test
    id: one part per kernel path or API, each walking its cases (milliseconds each).  A failed
    assertion does not stop the other parts — the failure names every failing part and, through
    each(), its case; any other error (a HIP error among them) ends the walk at once: nothing more
    is launched after it."""
    _dev()
    failed = []
    for part in _parts():
        try:
            part(tmp_path) if part.__name__ == "part_checkpoint" else part()
        except AssertionError as e:
            failed.append(f"{part.__name__}: {e}")
    assert not failed, "\n\n".join(failed)
