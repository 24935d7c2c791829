"""Output-space error on token samples on the GPU (include/awq_hip.h awq_output_error; DESIGN.md
§5.13): the MFMA kernels against float64 products put together in numpy from the test's own
reader of the packed layout, and the Python API on top of them.

  * exact data — every product and every partial sum is exact in fp32 in any order, so E must
    equal the float64 product bit for bit: pins the lane maps, the k order, the hi / lo split, the
    tails and the tile seams of both kernels;
  * random data — the header's accuracy contract, per element of E and for the row sums;
  * non-finite inputs, run-to-run determinism, guard bands and dirty buffers;
  * quantization_error(samples=) and quantize_layer_group(loss="output")."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_gpu_bounds import Call

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
_ids = lambda v: str(v).replace("torch.", "")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from awq_quantizer import _hip
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    return dev


def eps_k(K):
    return 2.0 ** -17 + K * 2.0 ** -22


# ---------------------------------------------------------------- the test's own reader (numpy)
def pack_fields(f: np.ndarray, bits: int) -> np.ndarray:
    """fields [R, n] (0 .. 2^bits - 1) -> int32 words [R, ceil(n bits / 32)], field j of a word at bit j * bits"""
    per = 32 // bits
    R, n = f.shape
    pad = (-n) % per
    f = np.pad(f.astype(np.uint64), ((0, 0), (0, pad))).reshape(R, -1, per)
    words = np.zeros(f.shape[:2], dtype=np.uint64)
    for j in range(per):
        words |= f[:, :, j] << np.uint64(j * bits)
    return words.astype(np.uint32).view(np.int32)


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
    """d = RN_f32(w^ - w), w^ = dq or RN_f32(dq / col_scale)"""
    with np.errstate(all="ignore"):
        wh = dq if col is None else (dq / col[None, :].astype(np.float32)).astype(np.float32)
        return (wh - w32).astype(np.float32)


def to_np32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().float().numpy()


# ---------------------------------------------------------------- running the entry
def strided(x: torch.Tensor, pad: int, dev) -> torch.Tensor:
    """x [T, K] on the device as a view with row stride K + pad (the gap holds NaN-free junk)"""
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


def run(dev, case, *, ref=True, err=True, pad=0, skew=False):
    from awq_quantizer import _hip
    w = skewed(case["w"], dev) if skew else case["w"].to(dev)
    x = skewed(case["x"], dev) if skew else (strided(case["x"], pad, dev) if pad else case["x"].to(dev))
    col = None if case["col"] is None else torch.from_numpy(case["col"]).to(dev)
    e_sq, r_sq, e = _hip.output_error(w, case["gs"], case["bits"], case["sym"],
                                      torch.from_numpy(case["qweight"]).to(dev), torch.from_numpy(case["qzeros"]).to(dev),
                                      torch.from_numpy(case["scales"].view(np.int16)).to(dev).view(F16), x, col,
                                      ref=ref, err=err)
    torch.cuda.synchronize(dev)
    return (e_sq.cpu().numpy(), None if r_sq is None else r_sq.cpu().numpy(), None if e is None else e.cpu().numpy())


def is_fast(case, pad=0, skew=False):
    return case["w"].dtype == BF16 and case["gs"] in (32, 64, 128, 256) and not skew and pad % 8 == 0


# ---------------------------------------------------------------- exact data
def exact_case(N, K, T, gs, bits, sym, dtype, col_pow2, seed):
    """scales = 1, q - z integers of at most 5 bits, w = m 2^-8 (m in [0, 255]: exact in bf16, fp16
    and fp32), x integers in [-2, 2], col_scale NULL or powers of two in [1/2, 2]: |d| < 64 on a
    2^-8 grid — up to 14 significant bits, so d_lo != 0 for most elements — and A = sum |d| |x| <
    512 * 64 * 2 = 2^16 on that grid: every partial sum fits fp32's 24 bits in any order."""
    rng = np.random.default_rng(seed)
    qmax = (1 << bits) - 1
    G = K // gs
    z = rng.integers(0, qmax + 1, size=(N, G))
    if bits == 4:
        q = rng.integers(0, qmax + 1, size=(N, K))
    else:   # the fields use all 8 bits, q - z stays within +-31
        q = np.clip(np.repeat(z, gs, axis=1) + rng.integers(-31, 32, size=(N, K)), 0, qmax)
    m = rng.integers(0, 256, size=(N, K))
    w = torch.from_numpy((m / 256.0).astype(np.float32)).to(dtype)
    x = torch.from_numpy(rng.integers(-2, 3, size=(T, K)).astype(np.float32)).to(dtype)
    col = (2.0 ** rng.integers(-1, 2, size=K)).astype(np.float32) if col_pow2 else None
    case = {"w": w, "x": x, "col": col, "gs": gs, "bits": bits, "sym": sym,
            "qweight": pack_fields(q, bits), "qzeros": pack_fields(z, bits),
            "scales": np.full((N, G), 0x3C00, dtype=np.uint16)}
    w32, x32 = to_np32(w), to_np32(x)
    assert np.array_equal(w32, (m / 256.0).astype(np.float32))
    d = d_of(w32, dequant_np(case["qweight"], case["qzeros"], case["scales"], bits, gs, K), col)
    d64, w64, x64 = d.astype(np.float64), w32.astype(np.float64), x32.astype(np.float64)
    case["E"], case["R"] = d64 @ x64.T, w64 @ x64.T
    A = np.abs(d64) @ np.abs(x64).T
    assert A.max() * 256 < 2 ** 24 and np.array_equal(d64 * 256, np.round(d64 * 256))
    return case


def check_exact(case, got, T):
    e_sq, r_sq, e = got
    tol = (T + 2) * 2.0 ** -24
    if e is not None:
        assert e.dtype == np.float32 and np.array_equal(e.astype(np.float64), case["E"])
    want = (case["E"] ** 2).sum(axis=1)
    assert np.all(np.abs(e_sq - want) <= tol * want), np.abs(e_sq / np.maximum(want, 1e-300) - 1).max()
    if r_sq is not None:
        want = (case["R"] ** 2).sum(axis=1)
        assert np.all(np.abs(r_sq - want) <= tol * want)


SHAPES = [(32, 32, 32), (33, 64, 1), (40, 128, 33), (72, 256, 70), (130, 512, 129), (260, 256, 300)]
EXACT = []
for _i, (_N, _K, _T) in enumerate(SHAPES):
    for _j, _gs in enumerate(g for g in (32, 64, 128, 256) if g <= _K):
        for _bits in (4, 8):
            _v = _i + _j + _bits // 8
            # symmetric, x_row_stride = K + 8 and col_scale alternate over the cases
            EXACT.append((_N, _K, _T, _gs, _bits, bool(_v & 1), 8 * ((_v >> 1) & 1), bool((_v >> 2) & 1) ^ bool(_j & 1)))


def each(fn, cases):
    """fn(dev, *case) for every case of one test, the case named in the failure it raises (one
    test id per kernel path rather than one per case: a case takes milliseconds)."""
    dev = _dev()
    for c in cases:
        try:
            fn(dev, *c)
        except AssertionError as e:
            raise AssertionError(f"case {_ids(c)}: {e}") from e


def test_exact_fast():
    """The fast kernel, every case of EXACT: E equals the float64 product exactly, err_sq / ref_sq
    within (T + 2) 2^-24; ref_sq and err NULL give the same err_sq bits."""
    def one(dev, N, K, T, gs, bits, sym, pad, col):
        case = exact_case(N, K, T, gs, bits, sym, BF16, col, seed=N + K + T + gs + bits)
        assert is_fast(case, pad)
        got = run(dev, case, pad=pad)
        check_exact(case, got, T)
        bare = run(dev, case, ref=False, err=False, pad=pad)
        assert bare[1] is None and bare[2] is None and np.array_equal(bare[0].view(np.int32), got[0].view(np.int32))

    each(one, EXACT)


GENERIC = [(33, 64, 1, 32, 4, False, 0, False), (40, 128, 33, 64, 8, True, 8, True), (72, 256, 70, 128, 4, True, 3, True),
           (130, 512, 129, 256, 8, False, 0, False), (260, 256, 300, 32, 4, False, 5, True)]


def test_exact_generic():
    """The generic kernel on exact data: fp16 and fp32 on five shapes (odd strides among them);
    group_size 8, 16 and 512, also for bf16; and bf16 with w and x one element past an aligned
    address, where E is identical to the fast kernel's."""
    def dtypes(dev, dtype, N, K, T, gs, bits, sym, pad, col):
        case = exact_case(N, K, T, gs, bits, sym, dtype, col, seed=N + K + T + bits)
        assert not is_fast(case, pad)
        got = run(dev, case, pad=pad)
        check_exact(case, got, T)
        bare = run(dev, case, ref=False, err=False, pad=pad)
        assert np.array_equal(bare[0].view(np.int32), got[0].view(np.int32))

    def group_sizes(dev, N, K, T, gs, bits):
        case = exact_case(N, K, T, gs, bits, False, BF16, True, seed=gs)
        assert not is_fast(case)
        check_exact(case, run(dev, case), T)

    def element_aligned(dev, N, K, T, gs, bits):
        case = exact_case(N, K, T, gs, bits, False, BF16, True, seed=N + bits)
        fast = run(dev, case)
        gen = run(dev, case, skew=True)
        assert is_fast(case) and not is_fast(case, skew=True)
        check_exact(case, fast, T)
        check_exact(case, gen, T)
        assert np.array_equal(fast[2].view(np.int32), gen[2].view(np.int32))

    each(dtypes, [(d, *c) for d in (F16, F32) for c in GENERIC])
    each(group_sizes, [(8, 64, 5, 8, 4), (20, 48, 17, 16, 8), (17, 1024, 9, 512, 4)])
    each(element_aligned, [(72, 256, 70, 64, 4), (130, 512, 129, 128, 8)])


# ---------------------------------------------------------------- random data against float64
def random_case(N, K, T, gs, bits, sym, dtype, seed, dev):
    from awq_quantizer.quantization import AWQQuantizer
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.02).to(dtype)
    x = torch.randn(T, K, generator=g).to(dtype)
    col = torch.exp((torch.rand(K, generator=g) * 2 - 1) * math.log(4.0)).numpy().astype(np.float32)
    q = AWQQuantizer(bits=bits, group_size=gs, symmetric=sym, device="cuda:0", logger_level="ERROR")
    r = q.quantize_packed(w.to(dev))
    return {"w": w, "x": x, "col": col, "gs": gs, "bits": bits, "sym": sym,
            "qweight": r["qweight"].cpu().numpy(), "qzeros": r["qzeros"].cpu().numpy(),
            "scales": r["scales"].cpu().view(torch.int16).numpy().view(np.uint16)}


def contract(case, got, T, K):
    """The header's bound per element of E and, by Cauchy-Schwarz, for the row sums.  Returns the
    measured maxima (|E - E_exact| / A, and the row sums' error over their bound)."""
    e_sq, r_sq, e = got
    eps = eps_k(K)
    w64, x64 = to_np32(case["w"]).astype(np.float64), to_np32(case["x"]).astype(np.float64)
    d64 = d_of(to_np32(case["w"]), dequant_np(case["qweight"], case["qzeros"], case["scales"], case["bits"],
                                             case["gs"], K), case["col"]).astype(np.float64)
    E, A = d64 @ x64.T, np.abs(d64) @ np.abs(x64).T
    assert np.all(np.abs(e - E) <= eps * A)
    rel = float((np.abs(e - E) / A).max())
    worst = 0.0
    for s, M, B in ((e_sq, E, A), (r_sq, w64 @ x64.T, np.abs(w64) @ np.abs(x64).T)):
        want, a2 = (M ** 2).sum(axis=1), (B ** 2).sum(axis=1)
        bound = 2 * eps * np.sqrt(a2 * want) + eps ** 2 * a2
        bound = bound + (T + 1) * 2.0 ** -24 * (want + bound)
        assert np.all(np.abs(s - want) <= bound)
        worst = max(worst, float((np.abs(s - want) / bound).max()))
    return rel, worst


RANDOM = [(72, 256, 70, 64, 4, False, BF16), (130, 512, 129, 128, 4, True, BF16), (72, 256, 70, 256, 8, False, BF16),
          (40, 128, 33, 32, 4, False, F16), (33, 64, 17, 16, 8, True, F32)]


def test_random_contract():
    """Random data against float64: the header's accuracy contract, per element and per row."""
    def one(dev, N, K, T, gs, bits, sym, dtype):
        case = random_case(N, K, T, gs, bits, sym, dtype, seed=N + K + bits, dev=dev)
        rel, worst = contract(case, run(dev, case), T, K)
        print(f"output_error {_ids(dtype)} ({N}, {K}, {T}) gs {gs} bits {bits}: max |E - E_exact| / A = {rel:.3e} "
              f"(eps_K = {eps_k(K):.3e}), row sums at {worst:.3e} of their bound")

    each(one, RANDOM)


# ---------------------------------------------------------------- non-finite, determinism
def test_non_finite():
    """A NaN weight and an inf sample reach exactly the sums that contain them (both kernels)."""
    each(_non_finite, [(False,), (True,)])


def _non_finite(dev, skew):
    N, K, T = 72, 256, 70
    case = exact_case(N, K, T, 64, 4, False, BF16, True, seed=11)
    clean = run(dev, case, skew=skew)
    bad_w = dict(case, w=case["w"].clone())
    bad_w["w"][5, 17] = float("nan")
    got = run(dev, bad_w, skew=skew)
    rows = np.arange(N) != 5
    assert not np.isfinite(got[0][5]) and not np.isfinite(got[1][5]) and not np.isfinite(got[2][5]).any()
    for g, c in zip(got, clean):
        assert np.array_equal(g[rows].view(np.int32), c[rows].view(np.int32))
    bad_x = dict(case, x=case["x"].clone())
    bad_x["x"][3, 9] = float("inf")
    got = run(dev, bad_x, skew=skew)
    cols = np.arange(T) != 3
    assert not np.isfinite(got[0]).any() and not np.isfinite(got[1]).any() and not np.isfinite(got[2][:, 3]).any()
    assert np.array_equal(got[2][:, cols].view(np.int32), clean[2][:, cols].view(np.int32))


def test_deterministic():
    dev = _dev()
    case = random_case(260, 256, 300, 64, 4, False, BF16, seed=3, dev=dev)
    a, b = run(dev, case), run(dev, case)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.int32), v.view(np.int32))


# ---------------------------------------------------------------- guard bands and dirty buffers
def test_guard_bands():
    """Every buffer out of a guard-band arena, outputs holding the fill: err_sq, ref_sq and err are
    fully written, nothing else is; N and T tails of both kernels ((130, 256, 129): 2 x 2 tiles)."""
    each(_guard_bands, [(BF16, 0, True, True), (BF16, 0, False, False), (BF16, 2, True, True), (F32, 4, True, False)])


def _guard_bands(dev, dtype, skew, ref, err):
    from awq_quantizer import _hip
    lib = _hip.load_library()
    N, K, T, gs, bits = 130, 256, 129, 64, 4
    case = exact_case(N, K, T, gs, bits, False, dtype, True, seed=7)
    want = run(dev, case, ref=ref, err=err, skew=bool(skew))
    nbytes = lib.awq_output_error_work_bytes(N, T)
    assert nbytes == 2 * 2 * N * 4
    c = Call(dev, seed=K + skew)
    wb = c.inp("w", case["w"], skew=skew, align=16)
    qb = c.inp("qweight", case["qweight"])
    zb = c.inp("qzeros", case["qzeros"])
    sb = c.inp("scales", case["scales"].view(np.int16))
    cb = c.inp("col_scale", case["col"])
    xb = c.inp("x", case["x"], skew=skew, align=16)
    kb = c.work("work", nbytes)
    eb = c.out("err_sq", want[0])
    rb = c.out("ref_sq", want[1]) if ref else None
    fb = c.out("err", want[2]) if err else None
    c.build()
    assert (dtype == BF16 and wb.addr % 16 == 0 and xb.addr % 16 == 0) == (dtype == BF16 and skew == 0)
    c.run(lambda: lib.awq_output_error(wb.ptr, _hip.AWQ_DTYPE[dtype], N, K, gs, bits, 0, qb.ptr, zb.ptr, sb.ptr, cb.ptr,
                                       xb.ptr, T, K, kb.ptr, eb.ptr, rb.ptr if rb else None, fb.ptr if fb else None,
                                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))


# ---------------------------------------------------------------- Python API
def _quantizer(**kw):
    from awq_quantizer.quantization import AWQQuantizer
    return AWQQuantizer(**dict(dict(bits=4, group_size=32, symmetric=False, device="cuda:0", logger_level="ERROR"), **kw))


def test_api_samples():
    dev = _dev()
    from awq_quantizer import _hip
    q = _quantizer(group_size=64)
    g = torch.Generator().manual_seed(21)
    w = (torch.randn(72, 256, generator=g) * 0.02).to(BF16)
    x = torch.randn(70, 256, generator=g)                       # fp32 on the CPU: converted to bf16
    res = q.quantize_packed(w.to(dev))
    plain = q.quantization_error(w, res)
    got = q.quantization_error(w, res, per_group=True, samples=x)
    e_sq, r_sq, _ = _hip.output_error(w.to(dev), 64, 4, False, res["qweight"], res["qzeros"], res["scales"],
                                      x.to(BF16).to(dev))
    assert torch.equal(got["row_output_sq"].view(torch.int32), e_sq.view(torch.int32))
    assert torch.equal(got["row_output_ref_sq"].view(torch.int32), r_sq.view(torch.int32))
    es, rs = float(e_sq.double().sum()), float(r_sq.double().sum())
    assert (got["output_sum_sq"], got["output_ref_sq"], got["output_tokens"]) == (es, rs, 70)
    assert got["output_rel_error"] == math.sqrt(es / rs) and got["output_snr_db"] == 10.0 * math.log10(rs / es)
    # without samples: today's keys and values
    assert set(plain) == {"numel", "nonfinite", "sum_abs", "sum_sq", "sum_w_sq", "mean_abs_error", "mse",
                          "max_abs_error", "snr_db", "input_scaled"}
    assert all(got[k] == v for k, v in plain.items())
    with pytest.raises(ValueError, match="samples"):
        q.quantization_error(w, res, samples=x[:, :128])
    with pytest.raises(ValueError, match="samples"):
        q.quantization_error(w, res, samples=x[0])


def test_api_input_scale():
    dev = _dev()
    q = _quantizer(scale_method="awq", search_grid=8)
    g = torch.Generator().manual_seed(22)
    w = (torch.randn(64, 128, generator=g) * 0.02).to(BF16)
    x = (torch.randn(48, 128, generator=g) * (1 + 3 * torch.rand(128, generator=g))).to(BF16)
    out = q.quantize_layer_group({"w": w}, x)
    res = out["results"]["w"]
    s = res["input_scale"].cpu().numpy()
    assert not np.all(s == 1.0)
    got = q.quantization_error(w, res, samples=x)
    assert got["input_scaled"] is True
    scales = res["scales"].cpu().view(torch.int16).numpy().view(np.uint16)
    dq = dequant_np(res["qweight"].cpu().numpy(), res["qzeros"].cpu().numpy(), scales, 4, 32, 128)
    d64 = d_of(to_np32(w), dq, s).astype(np.float64)
    x64, w64 = to_np32(x).astype(np.float64), to_np32(w).astype(np.float64)
    E, A = d64 @ x64.T, np.abs(d64) @ np.abs(x64).T
    want, a2, eps = (E ** 2).sum(), (A ** 2).sum(), eps_k(128)
    bound = 2 * eps * math.sqrt(a2 * want) + eps ** 2 * a2
    bound += (48 + 1 + 64) * 2.0 ** -24 * (want + bound)          # + the fp64 sum of 64 fp32 rows: exact; margin
    assert abs(got["output_sum_sq"] - want) <= bound
    ref = ((w64 @ x64.T) ** 2).sum()
    assert got["output_ref_sq"] == pytest.approx(ref, rel=2 * eps_k(128) * 10)


# seed 11: chosen on the CPU (the oracle's candidates of this construction, float64 losses, seeds
# 0 .. 11 tried): the minimum (candidate 3) and the runner-up differ by 43 x the contract's bound
SEARCH_SEED = 11


def _search_inputs():
    g = torch.Generator().manual_seed(SEARCH_SEED)
    ws = {"a": (torch.randn(64, 128, generator=g) * 0.02).to(BF16), "b": (torch.randn(96, 128, generator=g) * 0.02).to(BF16)}
    x = (torch.randn(48, 128, generator=g) * (0.25 + 4 * torch.rand(128, generator=g) ** 3)).to(BF16)
    return ws, x


def test_api_search():
    dev = _dev()
    from awq_quantizer import _hip
    q = _quantizer(scale_method="awq", search_grid=8)
    ws, x = _search_inputs()
    diag = q.quantize_layer_group(ws, x)
    out = q.quantize_layer_group(ws, x, loss="output")
    assert out["loss"] == "output" and "loss" not in diag and "diag_best" not in diag
    assert out["diag_best"] == diag["best"] and torch.equal(out["diag_losses"], diag["losses"])
    assert torch.equal(out["table"], diag["table"])
    table = out["table"]
    x64 = to_np32(x).astype(np.float64)
    want = np.zeros(8)
    bound = np.zeros(8)
    eps = eps_k(128)
    for i in range(8):                      # the GPU's own packed candidate, read by the numpy reader
        for name, w in ws.items():
            wd = w.to(dev)
            r = q._packed_outputs(wd)
            _hip.quantize_groups_scaled(wd, table[i], 32, 4, False, qweight=r["qweight"], qzeros=r["qzeros"],
                                        scales=r["scales"])
            scales = r["scales"].cpu().view(torch.int16).numpy().view(np.uint16)
            dq = dequant_np(r["qweight"].cpu().numpy(), r["qzeros"].cpu().numpy(), scales, 4, 32, 128)
            d64 = d_of(to_np32(w), dq, table[i].cpu().numpy()).astype(np.float64)
            E, A = d64 @ x64.T, np.abs(d64) @ np.abs(x64).T
            e2, a2 = (E ** 2).sum(), (A ** 2).sum()
            b = 2 * eps * math.sqrt(a2 * e2) + eps ** 2 * a2
            want[i] += e2
            bound[i] += b + (48 + 1) * 2.0 ** -24 * (e2 + b)
    losses = out["losses"].cpu().numpy()
    print("output losses", losses, "float64", want, "bounds", bound, "diag best", diag["best"], "output best", out["best"])
    assert np.all(np.abs(losses - want) <= bound)
    order = np.argsort(want, kind="stable")
    assert want[order[1]] - want[order[0]] > 10 * bound.max()       # the seed's margin
    assert out["best"] == int(order[0]) and out["ratio"] == out["best"] / 8
    assert losses[out["best"]] <= losses[0]
    assert torch.equal(out["input_scale"], table[out["best"]])
    for name in ws:
        assert torch.equal(out["results"][name]["input_scale"], out["input_scale"])
    # loss="diag" is today's call
    again = q.quantize_layer_group(ws, x, loss="diag")
    assert set(again) == set(diag) and again["best"] == diag["best"] and torch.equal(again["losses"], diag["losses"])
    for name in ws:
        for k in ("qweight", "qzeros", "scales", "input_scale"):
            assert torch.equal(again["results"][name][k], diag["results"][name][k])
    with pytest.raises(ValueError, match="samples"):
        q.quantize_layer_group(ws, x_mean=diag["input_scale"], x_sq=diag["input_scale"], loss="output")
    with pytest.raises(ValueError, match="loss"):
        q.quantize_layer_group(ws, x, loss="mse")
