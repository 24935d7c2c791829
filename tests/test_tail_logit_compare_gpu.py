"""awq_logit_compare on the GPU (include/awq_hip.h) against a float64 torch
restatement of its definitions.

Every call places its inputs and outputs in a guard-band arena (tests/guard_arena.py), runs from
both fill polarities with the outputs holding the fill, and passes iff the guards are intact, every
requested output is fully written and every output whose pointer is NULL (or that the call does not
own: the nll outputs without targets) still holds the fill.  Each test walks its cases and names
the failing ones.

Bounds.  nll and kl are held to the header's contract, computed here from its constants:
  D = 104, c0 = 48, C = 4 ceil(ceil(V / 8) / 256) + 20, E = (D + C + c0) 2^-24
  |nll - nll64| <= E + 2^-23 |lse| + 2^-24 |nll|
  |kl - kl64|   <= 2 E (1 + M1) + 3 2^-24 (M1 + |lse_r| + |lse_q|),  M1 = sum_v p_v |a_v - b_v|
argmax is exact (lowest index attaining the maximum).  Measured max error / bound on an MI355X over
the random cases: see DESIGN.md §5.16 (printed by test_shapes_and_dtypes).
"""
import ctypes
import math

import pytest
import torch

import stream_gate
from guard_arena import Arena

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
OUTS = ("nll_ref", "nll_q", "kl", "argmax_ref", "argmax_q")
D_CONST, C0 = 104.0, 48.0


def _dev():
    from awq_quantizer import _hip
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    return dev


def chain(V):
    return 4 * math.ceil(math.ceil(V / 8) / 256) + 20


# ------------------------------------------------------------------ the oracle
def oracle(ref, q, targets):
    """float64 restatement on the decoded inputs.  -> dict of float64 / int64 tensors and the bounds."""
    V = ref.shape[1]
    ar = torch.arange(V)

    def side(x):
        x = x.double()
        bad = ~torch.isfinite(x).all(-1)
        x0 = torch.where(bad[:, None], torch.zeros(()).double(), x)
        lsm = torch.log_softmax(x0, -1)
        lse = torch.logsumexp(x0, -1)
        mx = x0.max(-1, keepdim=True).values
        am = torch.where(x0 == mx, ar, V).min(-1).values
        return x0, lsm, lse, torch.where(bad, -1, am), bad

    E = (D_CONST + chain(V) + C0) * 2.0 ** -24
    a, la, lse_r, am_r, bad_r = side(ref)
    out = {"argmax_ref": am_r, "bad_r": bad_r}

    def nll(x, lsm, lse, bad):
        if targets is None:
            return None, None
        t = targets
        safe = t.clamp(0, V - 1)[:, None]
        v = -lsm.gather(1, safe)[:, 0]
        v = torch.where(t < 0, torch.zeros(()).double(), v)
        v = torch.where((t >= V) | (bad & (t >= 0)), torch.full((), float("nan")).double(), v)
        return v, E + 2.0 ** -23 * lse.abs() + 2.0 ** -24 * v.abs()

    out["nll_ref"], out["nll_ref_bound"] = nll(a, la, lse_r, bad_r)
    if q is not None:
        b, lb, lse_q, am_q, bad_q = side(q)
        out["argmax_q"], out["bad_q"] = am_q, bad_q
        out["nll_q"], out["nll_q_bound"] = nll(b, lb, lse_q, bad_q)
        p = la.exp()
        kl = (p * (la - lb)).sum(-1)
        M1 = (p * (a - b).abs()).sum(-1)
        out["kl"] = torch.where(bad_r | bad_q, torch.full((), float("nan")).double(), kl)
        out["kl_bound"] = 2 * E * (1 + M1) + 3 * 2.0 ** -24 * (M1 + lse_r.abs() + lse_q.abs())
    return out


# ------------------------------------------------------------------ one call in an arena
def strided(x, stride, pad):
    """[T, V] -> the flat buffer of (T - 1) * stride + V elements, the padding holding `pad`."""
    T, V = x.shape
    flat = torch.full(((T - 1) * stride + V,), pad, dtype=x.dtype)
    for t in range(T):
        flat[t * stride: t * stride + V] = x[t]
    return flat


def call(dev, ref, q=None, targets=None, *, sr=None, sq=None, pad=float("nan"), skew=0, outs=OUTS, seed=1,
         complement=False, ordered=None):
    """-> {output name: CPU tensor} of the outputs that were requested.  ref / q: CPU [T, V] of one dtype."""
    from awq_quantizer import _hip
    lib = _hip.load_library()
    T, V = ref.shape
    es = ref.element_size()
    sr = V if sr is None else sr
    sq = V if sq is None else sq
    arena = Arena(Arena.required([((T - 1) * max(sr, sq) + V) * es] * 2 + [T * 8] * 6), device=dev)
    r_ref = arena.place(((T - 1) * sr + V) * es, skew=skew * es, name="ref", untouched=True)
    r_q = arena.place(((T - 1) * sq + V) * es, skew=skew * es, name="q", untouched=True) if q is not None else None
    r_t = arena.place(T * 8, name="targets", untouched=True) if targets is not None else None
    owned = {"nll_ref": targets is not None, "nll_q": targets is not None and q is not None, "kl": q is not None,
             "argmax_ref": True, "argmax_q": q is not None}
    regions = {k: arena.place(T * 4, name=k, untouched=not owned[k]) for k in outs}
    arena.fill(seed, complement)
    r_ref.store(strided(ref, sr, pad))
    if q is not None:
        r_q.store(strided(q, sq, pad))
    if targets is not None:
        r_t.store(targets)
    P = ctypes.c_void_p

    def ptr(r):
        return P(r.data_ptr()) if r is not None else P(0)

    def launch():
        stream = P(torch.cuda.current_stream(dev).cuda_stream)
        rc = lib.awq_logit_compare(ptr(r_ref), ptr(r_q), _hip.AWQ_DTYPE[ref.dtype], T, V, sr, sq, ptr(r_t),
                                   *[ptr(regions.get(k)) for k in OUTS], stream)
        assert rc == 0, _hip.last_error()

    if ordered is None:
        launch()
    else:                                     # inputs stale until the gate has passed (tests/stream_gate.py)
        launch()                              # the kernel's code loads at its first launch
        ins = [r.u8 for r in (r_ref, r_q, r_t) if r is not None]
        for k in regions.values():            # the warm-up's outputs go back to the fill
            k.u8.copy_(arena._fill[k.start:k.end])
        stream_gate.run_tensors(ordered, ins, launch)
    arena.check()
    return {k: r.load(torch.float32 if k in ("nll_ref", "nll_q", "kl") else torch.int32)
            for k, r in regions.items() if owned[k]}


def check(got, want, label, worst=None):
    """Every requested output against the oracle; returns a list of complaints."""
    bad = []
    for k, g in got.items():
        w = want[k]
        if k.startswith("argmax"):
            if not torch.equal(g.to(torch.int64), w):
                bad.append(f"{label}: {k} differs at rows {torch.nonzero(g.to(torch.int64) != w).reshape(-1)[:4].tolist()}")
            continue
        nan_w = torch.isnan(w)
        if not torch.equal(torch.isnan(g), nan_w):
            bad.append(f"{label}: {k} NaN pattern differs")
            continue
        ok = ~nan_w
        err = (g.double() - w)[ok].abs()
        ratio = err / want[k + "_bound"][ok]
        if ratio.numel() and float(ratio.max()) > 1.0:
            bad.append(f"{label}: {k} error / bound {float(ratio.max()):.3g} (error {float(err.max()):.3g})")
        if worst is not None and ratio.numel():
            key = (k.split("_")[0], label.split()[0])
            worst[key] = max(worst.get(key, 0.0), float(ratio.max()))
    return bad


def both_fills(dev, ref, q, targets, label, **kw):
    """The call from both fill polarities: identical bits, and the oracle.  -> (outputs, complaints)."""
    a = call(dev, ref, q, targets, seed=3, complement=False, **kw)
    b = call(dev, ref, q, targets, seed=3, complement=True, **kw)
    bad = [f"{label}: {k} depends on what the buffers held" for k in a if not same_bits(a[k], b[k])]
    return a, bad


def same_bits(x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


def random_case(T, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    ref = (torch.randn(T, V, generator=g) * 4).to(dtype)
    q = (ref.float() + torch.randn(T, V, generator=g) * 0.3).to(dtype)
    targets = torch.randint(0, V, (T,), generator=g)
    return ref, q, targets


# ------------------------------------------------------------------ the tests
def test_shapes_and_dtypes():
    """V: one lane, one chunk, ragged tails, more than one chunk per thread (2 059, 4 099 > 256 x 8 x 2);
    T: one row, a few, more than a wave of rows.  Random logits N(0, 4^2), q = ref + N(0, 0.3^2)."""
    dev = _dev()
    bad, worst = [], {}
    for name, dtype in DTYPES.items():
        for V in (1, 7, 8, 255, 256, 2059, 4099):
            for T in (1, 3, 130):
                ref, q, t = random_case(T, V, dtype, 1000 * V + T)
                label = f"{name} T={T} V={V}"
                got, b = both_fills(dev, ref, q, t, label)
                bad += b + check(got, oracle(ref, q, t), label, worst)
    for (what, name), r in sorted(worst.items()):
        print(f"max error / bound  {what:4s} {name}: {r:.4f}")
    assert not bad, "\n".join(bad)


def test_optional_arguments():
    """q present / NULL, targets present / NULL, every output pointer on and off: what is written is
    the full call's bits, what is not requested or not owned keeps the fill (arena.check)."""
    dev = _dev()
    ref, q, t = random_case(3, 2059, torch.bfloat16, 7)
    full = call(dev, ref, q, t)
    bad = check(full, oracle(ref, q, t), "full")
    combos = [(q, t, OUTS), (None, t, OUTS), (q, None, OUTS), (None, None, OUTS), (q, t, ())]
    combos += [(q, t, tuple(o for o in OUTS if o != drop)) for drop in OUTS]
    combos += [(q, t, (only,)) for only in OUTS]
    for qq, tt, outs in combos:
        label = f"q={'on' if qq is not None else 'NULL'} targets={'on' if tt is not None else 'NULL'} outs={outs}"
        got, b = both_fills(dev, ref, qq, tt, label, outs=outs)
        bad += b
        for k, v in got.items():
            if not same_bits(v, full[k]):
                bad.append(f"{label}: {k} differs from the full call's bits")
        want_keys = {k for k in outs if (k in ("nll_ref", "argmax_ref") or qq is not None)
                     and (not k.startswith("nll") or tt is not None)}
        if set(got) != want_keys:
            bad.append(f"{label}: outputs {sorted(got)} != {sorted(want_keys)}")
    assert not bad, "\n".join(bad)


def test_strides_alignment_and_paths_give_the_same_bits():
    """Row strides V, V + 8, V + 3 and the next multiple of 8 with the padding NaN and +inf, bases
    offset by one element: the 16-B path (aligned base, stride % 8 == 0, fp32 % 4) and the
    element-aligned path give the bits of the contiguous call, and no padding leaks."""
    dev = _dev()
    bad = []
    for name, dtype in DTYPES.items():
        for V in (256, 2059):
            ref, q, t = random_case(3, V, dtype, V)
            base = call(dev, ref, q, t)
            bad += check(base, oracle(ref, q, t), f"{name} V={V} contiguous")
            up8 = (V + 8) // 8 * 8
            for sr, sq in ((V + 8, V + 8), (V + 3, V + 3), (up8, up8), (up8, V + 3), (V + 3, up8 + 8)):
                for pad in (float("nan"), float("inf")):
                    for skew in (0, 1):
                        label = f"{name} V={V} strides {sr}/{sq} pad {pad} base + {skew}"
                        got = call(dev, ref, q, t, sr=sr, sq=sq, pad=pad, skew=skew)
                        bad += [f"{label}: {k} differs from the contiguous call's bits" for k in got
                                if not same_bits(got[k], base[k])]
    assert not bad, "\n".join(bad)


def _poison(x, row, col, value):
    y = x.clone()
    y[row, col] = value
    return y


def test_numeric_cases():
    dev = _dev()
    bad = []
    V = 2059
    g = torch.Generator().manual_seed(5)
    t = torch.randint(0, V, (4,), generator=g)
    # rows with spread +-80 around a large offset: without the max subtraction exp overflows
    for name, dtype, off in (("fp32", torch.float32, 1e4), ("bf16", torch.bfloat16, 3e4)):
        ref = (off + (torch.rand(4, V, generator=g) * 160 - 80)).to(dtype)
        q = (ref.float() + torch.randn(4, V, generator=g)).to(dtype)
        got, b = both_fills(dev, ref, q, t, f"{name} offset {off:g}")
        bad += b + check(got, oracle(ref, q, t), f"{name} offset {off:g}")
        if not bool(torch.isfinite(got["nll_ref"]).all() and torch.isfinite(got["kl"]).all()):
            bad.append(f"{name} offset {off:g}: non-finite outputs")
    for name, dtype in DTYPES.items():
        # one dominant logit: nll ~ 0 and kl ~ 0
        ref = torch.zeros(3, V)
        ref[:, 77] = 60.0
        ref = ref.to(dtype)
        tt = torch.full((3,), 77)
        got = call(dev, ref, ref.clone(), tt)
        bad += check(got, oracle(ref, ref, tt), f"{name} dominant")
        if float(got["nll_ref"].abs().max()) > 1e-6 or float(got["kl"].abs().max()) != 0.0:
            bad.append(f"{name} dominant: nll {got['nll_ref'].tolist()} kl {got['kl'].tolist()}")
        # uniform rows: nll = log V, argmax 0 by the tie rule
        ref = torch.full((3, V), 1.5).to(dtype)
        got = call(dev, ref, ref.clone(), tt)
        want = oracle(ref, ref, tt)
        bad += check(got, want, f"{name} uniform")
        if got["argmax_ref"].tolist() != [0, 0, 0] or got["argmax_q"].tolist() != [0, 0, 0]:
            bad.append(f"{name} uniform: argmax {got['argmax_ref'].tolist()}")
        if float((got["nll_ref"].double() - math.log(V)).abs().max()) > float(want["nll_ref_bound"].max()):
            bad.append(f"{name} uniform: nll is not log V")
        # deliberate ties at the first, middle and last index, in both matrices
        ref, q, _ = random_case(5, V, dtype, 11)
        top = float(ref.float().max()) + 1
        for row, cols in enumerate(((0, 1000), (1000, V - 1), (0, V - 1), (7, 8, 9), (V - 2, V - 1))):
            for c in cols:
                ref[row, c] = top
                q[row, V - 1 - c] = top
        got = call(dev, ref, q, None)
        bad += check(got, oracle(ref, q, None), f"{name} ties")
        if got["argmax_ref"].tolist() != [0, 1000, 0, 7, V - 2]:
            bad.append(f"{name} ties: argmax_ref {got['argmax_ref'].tolist()}")
        if got["argmax_q"].tolist() != [V - 1 - 1000, 0, 0, V - 10, 0]:
            bad.append(f"{name} ties: argmax_q {got['argmax_q'].tolist()}")
        # identical matrices: kl == +0, nll_q == nll_ref, argmax equal, bit for bit
        ref, _, t5 = random_case(5, 4099, dtype, 13)
        got = call(dev, ref, ref.clone(), t5)
        if not (same_bits(got["kl"], torch.zeros(5)) and same_bits(got["nll_q"], got["nll_ref"])
                and torch.equal(got["argmax_q"], got["argmax_ref"])):
            bad.append(f"{name} identical: kl {got['kl'].tolist()}")
        # targets -1: +0 nll, nothing else moves; targets >= V: NaN nll
        ref, q, t5 = random_case(5, 255, dtype, 17)
        base = call(dev, ref, q, t5)
        t_mix = t5.clone()
        t_mix[1], t_mix[3], t_mix[4] = -1, 255, 1 << 40
        got = call(dev, ref, q, t_mix)
        bad += check(got, oracle(ref, q, t_mix), f"{name} targets")
        for k in ("nll_ref", "nll_q"):
            if not (same_bits(got[k][1:2], torch.zeros(1)) and bool(torch.isnan(got[k][3:]).all())
                    and same_bits(got[k][[0, 2]], base[k][[0, 2]])):
                bad.append(f"{name} targets: {k} {got[k].tolist()}")
        for k in ("kl", "argmax_ref", "argmax_q"):
            if not same_bits(got[k], base[k]):
                bad.append(f"{name} targets: {k} moved")
        # a non-finite row in ref only / q only: NaN and -1 there, the neighbours' bits unchanged
        ref, q, t5 = random_case(5, 2059, dtype, 19)
        base = call(dev, ref, q, t5)
        for value in (float("nan"), float("inf"), float("-inf")):
            for where in ("ref", "q"):
                r2 = _poison(ref, 2, 1234, value) if where == "ref" else ref
                q2 = _poison(q, 2, 2058, value) if where == "q" else q
                label = f"{name} {value} in {where}"
                got = call(dev, r2, q2, t5)
                bad += check(got, oracle(r2, q2, t5), label)
                rows = [0, 1, 3, 4]
                bad += [f"{label}: {k} of a neighbour moved" for k in got if not same_bits(got[k][rows], base[k][rows])]
                hit, kept = ("nll_ref", "argmax_ref"), ("nll_q", "argmax_q")
                if where == "q":
                    hit, kept = kept, hit
                if not (math.isnan(float(got[hit[0]][2])) and int(got[hit[1]][2]) == -1 and math.isnan(float(got["kl"][2]))):
                    bad.append(f"{label}: row 2 gives {[float(got[k][2]) for k in got]}")
                if not all(same_bits(got[k][2:3], base[k][2:3]) for k in kept):
                    bad.append(f"{label}: the other matrix's outputs moved")
    assert not bad, "\n".join(bad)


def test_determinism_and_row_independence():
    dev = _dev()
    bad = []
    for name, dtype in DTYPES.items():
        ref, q, t = random_case(200, 2059, dtype, 23)
        whole = call(dev, ref, q, t)
        again = call(dev, ref, q, t, seed=9)
        part = call(dev, ref[:130].contiguous(), q[:130].contiguous(), t[:130].contiguous())
        bad += [f"{name}: {k} differs between two runs" for k in whole if not same_bits(whole[k], again[k])]
        bad += [f"{name}: {k} of T = 130 differs from the first 130 rows of T = 200" for k in whole
                if not same_bits(whole[k][:130], part[k])]
    assert not bad, "\n".join(bad)


def test_rows_beyond_a_capped_grid():
    """The grid is capped (65 536 workgroups); the diagnostics build lowers the cap so that 7 rows
    take up to 7 trips of the row loop: the uncapped call's bits."""
    from awq_quantizer import _hip
    dev = _dev()
    bad = []
    ref, q, t = random_case(7, 2059, torch.bfloat16, 29)
    base = call(dev, ref, q, t)
    bad += check(base, oracle(ref, q, t), "uncapped")
    for cap in (1, 2, 3):
        with _hip.tuning(max_blocks=cap):
            got, b = both_fills(dev, ref, q, t, f"max_blocks={cap}")
        bad += b + [f"max_blocks={cap}: {k} differs from the uncapped call's bits" for k in got
                    if not same_bits(got[k], base[k])]
    assert not bad, "\n".join(bad)


def test_off_the_default_stream():
    """Behind tests/stream_gate.py's gate on a non-blocking stream: the launch is on the caller's
    stream (a launch on stream 0 would have read the stale complement of its inputs)."""
    dev = _dev()
    bad = []
    cases = [("bf16 16-B path", torch.bfloat16, 256, 0), ("fp32 element path", torch.float32, 2059, 1)]
    want = {}
    for label, dtype, V, skew in cases:
        ref, q, t = random_case(3, V, dtype, 31)
        want[label] = (ref, q, t, call(dev, ref, q, t, skew=skew))
    with stream_gate.ordered(dev) as st:
        for label, dtype, V, skew in cases:
            st.case = label
            ref, q, t, base = want[label]
            got = call(dev, ref, q, t, skew=skew, ordered=st)
            bad += [f"{label}: {k} differs from the default-stream bits" for k in got if not same_bits(got[k], base[k])]
        assert st.gates == len(cases)
    assert not bad, "\n".join(bad)


def test_python_wrappers():
    """_hip.logit_compare on row-strided views and evaluation.compare_logits' aggregates."""
    from awq_quantizer import _hip
    from awq_quantizer.evaluation import aggregate, compare_logits
    dev = _dev()
    ref, q, t = random_case(6, 255, torch.float16, 37)
    t[2] = -1
    base = call(dev, ref, q, t)
    wide_r = torch.full((6, 300), float("nan"), dtype=torch.float16, device=dev)
    wide_q = torch.full((6, 264), float("inf"), dtype=torch.float16, device=dev)
    wide_r[:, 3:258] = ref.to(dev)
    wide_q[:, :255] = q.to(dev)
    got = compare_logits(wide_r[:, 3:258], wide_q[:, :255], t)
    for k in OUTS:
        assert same_bits(got[k].cpu(), base[k]), k
    want = aggregate({k: base[k] for k in OUTS}, t)
    for k, v in want.items():              # (the device's and the host's fp64 means may differ in the last bit)
        assert got[k] == v or math.isclose(got[k], v, rel_tol=1e-12), k
    assert got["n_tokens_scored"] == 5
    single = compare_logits(ref.to(dev))
    assert single["nll_ref"] is None and single["kl"] is None and same_bits(single["argmax_ref"].cpu(), base["argmax_ref"])
    with pytest.raises(ValueError):
        _hip.logit_compare(ref.to(dev), q.to(dev).float())
    with pytest.raises(_hip.HipUnavailable):
        compare_logits(ref)                                  # a CPU tensor: there is no CPU fallback
