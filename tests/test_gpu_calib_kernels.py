"""The calibration pass' kernels on the GPU (include/awq_hip.h awq_act_stats_accum,
awq_rmsnorm_stats, awq_swiglu_stats; awq_quantizer/calibration/stats.py StatsAccumulator).

  * the running sums of any chunking are the bits of awq_act_stats (and of the CPU oracle's
    act_stats) on the concatenated rows;
  * the norm's output is the bits of the numpy float32 restatement below, which follows the
    summation order the header documents; its statistics are the oracle's on that output;
  * the SwiGLU product is within 1 ulp of the dtype of RN_D(RN_D(silu64(g)) * u) evaluated in
    float64 at every element (bf16 / fp16: the fp32 evaluation is within a few 2^-24 of the exact
    value, far inside half an ulp except at a rounding boundary, where the neighbour is allowed),
    its statistics exactly the oracle's on the output that was written;
  * every entry, out of a guard-band arena on both fill polarities, writes its outputs and nothing
    else, with outputs, workspaces and accumulators sized exactly as the header documents.
NaN results are compared as NaN (no definition here pins a payload)."""
import ctypes

import numpy as np
import pytest
import torch

from guard_arena import Arena
from oracle import awq_oracle as orc

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF16, F16, F32]
_ids = lambda v: str(v).replace("torch.", "")
EINVAL = 1


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from awq_quantizer import _hip
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    return dev


def _hipmod():
    from awq_quantizer import _hip
    return _hip


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """fp32 vectors: equal bits, or NaN in both."""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    ok = (a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
    return bool(ok.all())


def same_values(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Tensors of one dtype: equal bits, or NaN in both."""
    a, b = a.detach().cpu(), b.detach().cpu()
    it = torch.int32 if a.dtype == F32 else torch.int16
    ok = (a.contiguous().view(it) == b.contiguous().view(it)) | (torch.isnan(a) & torch.isnan(b))
    return bool(ok.all())


def rows(T, K, dtype, seed, specials=False):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, K, generator=g) * 2.0).to(dtype)
    if specials and K >= 8:
        x[:, 1] = -0.0
        x[T // 2, 2] = float("inf")
        x[T // 3, 3] = float("nan")
        x[0, 4] = float("-inf")
    return x


def finish(hip, acc_abs, acc_sq, T):
    return hip.column_mean(acc_abs, T), hip.column_mean(acc_sq, T)


# ---------------------------------------------------------------- awq_act_stats_accum
CHUNKS = ([256, 512, 37], [1], [255], [257], [256, 256])
KS = (8, 12, 40)      # the 16-B path; K % 8 != 0: one lane per column; one 16-B chunk past the 32-column tile


def _accum_chunks(hip, chunks, K, dev):
    a = torch.zeros(K, dtype=torch.float64, device=dev)
    s = torch.zeros(K, dtype=torch.float64, device=dev)
    before = 0
    for c in chunks:
        hip.act_stats_accum(c, before, a, s)
        before += c.shape[0]
    return finish(hip, a, s, before)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_accum_equals_act_stats_of_the_concatenation(dtype, K):
    dev, hip = _dev(), _hipmod()
    for n, sizes in enumerate(CHUNKS):
        T = sum(sizes)
        x = rows(T, K, dtype, 100 + n, specials=True)
        ref_m, ref_s = orc.act_stats(x)
        xd = x.to(dev)
        one_m, one_s = hip.act_stats(xd)
        assert same_bits(one_m, ref_m) and same_bits(one_s, ref_s)
        # contiguous chunks
        got = _accum_chunks(hip, list(torch.split(xd, sizes)), K, dev)
        assert same_bits(got[0], ref_m) and same_bits(got[1], ref_s), (sizes, "contiguous")
        # a view with row_stride = K + 8
        wide = torch.full((T, K + 8), 7.0, dtype=dtype, device=dev)
        wide[:, :K] = xd
        got = _accum_chunks(hip, list(torch.split(wide[:, :K], sizes)), K, dev)
        assert same_bits(got[0], ref_m) and same_bits(got[1], ref_s), (sizes, "strided")
        # an element-aligned (not 16-B aligned) pointer
        flat = torch.empty(T * K + 8, dtype=dtype, device=dev)
        off = 1 if flat.data_ptr() % 16 == 0 else 0
        view = flat[off:off + T * K].view(T, K)
        view.copy_(xd)
        assert view.data_ptr() % 16 != 0
        got = _accum_chunks(hip, list(torch.split(view, sizes)), K, dev)
        assert same_bits(got[0], ref_m) and same_bits(got[1], ref_s), (sizes, "element-aligned")


def test_accum_refuses_a_partial_block_before_it():
    dev, hip = _dev(), _hipmod()
    lib = hip.load_library()
    x = rows(64, 8, BF16, 1).to(dev)
    work = torch.zeros(hip.calib_work_size(64, 8), dtype=torch.float64, device=dev)
    a = torch.full((8,), 3.0, dtype=torch.float64, device=dev)
    s = torch.full((8,), 5.0, dtype=torch.float64, device=dev)
    rc = lib.awq_act_stats_accum(hip.ptr(x), hip.AWQ_DTYPE[BF16], 64, 8, 8, 100, hip.ptr(work), hip.ptr(a), hip.ptr(s),
                                 _stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == EINVAL and "tokens_before" in hip.last_error()
    assert bool((a == 3.0).all()) and bool((s == 5.0).all()) and bool((work == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_stats_accumulator_any_chunking(dtype):
    dev, hip = _dev(), _hipmod()
    from awq_quantizer.calibration import StatsAccumulator
    sizes = [100, 300, 7, 256, 1]
    for K in (40, 12):
        x = rows(sum(sizes), K, dtype, 7, specials=True)
        xd = x.to(dev)
        acc = StatsAccumulator(K, dev)
        for c in torch.split(xd, sizes):
            acc.add(c)
        m, s = acc.finish()
        whole_m, whole_s = hip.act_stats(xd)
        ref_m, ref_s = orc.act_stats(x)
        assert same_bits(m, whole_m) and same_bits(s, whole_s)
        assert same_bits(m, ref_m) and same_bits(s, ref_s)


# ---------------------------------------------------------------- awq_rmsnorm_stats
def to_dtype(a: np.ndarray, dtype) -> np.ndarray:
    """RN_D of a float32 array, as float32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).float().numpy()


def rmsnorm_ref(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """include/awq_hip.h awq_rmsnorm_stats in numpy float32, one rounding per line."""
    dtype = x.dtype
    xf, wf = x.float().numpy(), w.float().numpy()
    T, H = xf.shape
    nch = (H + 7) // 8
    nj = (nch + 63) // 64
    with np.errstate(all="ignore"):
        sq = np.zeros((T, nj * 64 * 8), dtype=np.float32)
        sq[:, :H] = xf * xf                                    # RN_f32(x^2); elements past H add +0
        sq = sq.reshape(T, nj, 64, 8)
        cs = np.zeros((T, nj, 64), dtype=np.float32)
        for j in range(8):                                     # a chunk's 8 elements in order from +0
            cs = cs + sq[:, :, :, j]
        slot = np.zeros((T, 64), dtype=np.float32)
        for j in range(nj):                                    # slot l: chunks l, l + 64, ... ascending
            slot = slot + cs[:, j, :]
        lanes = np.arange(64)
        for o in (1, 2, 4, 8, 16, 32):                         # the pairwise tree, adjacent pairs first
            slot = slot + slot[:, lanes ^ o]
        v = slot[:, 0]
        m = (v / np.float32(H)).astype(np.float32) + np.float32(eps)
        r = np.float32(1.0) / np.sqrt(m).astype(np.float32)
        h = to_dtype(xf * r[:, None], dtype)
        out = to_dtype(wf[None, :] * h, dtype)
    return torch.from_numpy(out).to(dtype)


NORM_H = (8, 128, 520, 4096, 12)   # 520: one chunk past the 512 elements a wave covers in one step; 12: no 16-B path
NORM_T = (1, 37, 256, 300)


def norm_case(T, H, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, H, generator=g) * 1.5).to(dtype)
    w = (1.0 + 0.2 * torch.randn(H, generator=g)).to(dtype)
    if T >= 37:
        x[3] = 0.0                        # r = 1 / sqrt(eps)
        x[5, H // 2] = float("inf")      # r = 0: inf * 0 = NaN, the rest of the row 0
    return x, w


@pytest.mark.parametrize("H", NORM_H)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_rmsnorm_stats(dtype, H):
    dev, hip = _dev(), _hipmod()
    eps = 1e-5
    for T in NORM_T:
        x, w = norm_case(T, H, dtype, 10 * H + T)
        ref = rmsnorm_ref(x, w, eps)
        ref_m, ref_s = orc.act_stats(ref)
        xd, wd = x.to(dev), w.to(dev)
        a = torch.zeros(H, dtype=torch.float64, device=dev)
        s = torch.zeros(H, dtype=torch.float64, device=dev)
        out = hip.rmsnorm_stats(xd, wd, eps, 0, a, s)
        assert same_values(out, ref), (T, "out")
        m, q = finish(hip, a, s, T)
        assert same_bits(m, ref_m) and same_bits(q, ref_s), (T, "stats")
        alone = hip.rmsnorm_stats(xd, wd, eps)               # acc_* = NULL
        assert same_values(alone, ref), (T, "norm alone")
        if T == 300:                                         # two calls [256, 44] = one call of 300
            a.zero_()
            s.zero_()
            o1 = hip.rmsnorm_stats(xd[:256], wd, eps, 0, a, s)
            o2 = hip.rmsnorm_stats(xd[256:], wd, eps, 256, a, s)
            assert same_values(torch.cat([o1, o2]), ref)
            m2, q2 = finish(hip, a, s, T)
            assert same_bits(m2, ref_m) and same_bits(q2, ref_s), "two calls"


def test_rmsnorm_zero_row_and_inf_row_values():
    dev, hip = _dev(), _hipmod()
    x, w = norm_case(37, 128, F32, 5)
    out = hip.rmsnorm_stats(x.to(dev), w.to(dev), 1e-6).cpu()
    assert bool((out[3] == 0).all())
    assert bool(torch.isnan(out[5, 64])) and bool((out[5, :64] == 0).all())
    expect = torch.nn.functional.rms_norm(x[:3], (128,), w, 1e-6)
    assert torch.allclose(out[:3], expect, rtol=1e-5, atol=1e-6)


def test_rmsnorm_refuses_aliasing_and_partial_blocks():
    dev, hip = _dev(), _hipmod()
    lib = hip.load_library()
    x = torch.ones(16, 8, dtype=F32, device=dev)
    w = torch.ones(8, dtype=F32, device=dev)
    work = torch.zeros(hip.calib_work_size(16, 8, norm=True), dtype=torch.float64, device=dev)
    args = (hip.AWQ_DTYPE[F32], 16, 8, hip.ptr(w), 1e-6)
    assert lib.awq_rmsnorm_stats(hip.ptr(x), *args, hip.ptr(x), 0, hip.ptr(work), None, None, _stream(dev)) == EINVAL
    out = torch.full((16, 8), 9.0, dtype=F32, device=dev)
    a = torch.zeros(8, dtype=torch.float64, device=dev)
    assert lib.awq_rmsnorm_stats(hip.ptr(x), *args, hip.ptr(out), 7, hip.ptr(work), hip.ptr(a), hip.ptr(a),
                                 _stream(dev)) == EINVAL
    torch.cuda.synchronize(dev)
    assert bool((out == 9.0).all()) and bool((a == 0).all())


# ---------------------------------------------------------------- awq_swiglu_stats
FMT = {BF16: (8, -133, float(torch.finfo(BF16).max)), F16: (11, -24, 65504.0)}


def round64(x: np.ndarray, dtype) -> np.ndarray:
    """RN_D of float64 values in one rounding (float64 result)."""
    mant, qmin, maxv = FMT[dtype]
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        _, e = np.frexp(x)
        q = np.exp2(np.maximum(e - mant, qmin).astype(np.float64))
        y = np.rint(x / q) * q
        y = np.where(np.abs(y) > maxv, np.sign(y) * np.inf, y)
    return np.where(np.isfinite(x), y, x)


def order_key(t: torch.Tensor) -> np.ndarray:
    """Values of a 16-bit or 32-bit float dtype on an integer line: neighbours differ by 1."""
    if t.dtype == F32:
        b = t.contiguous().view(torch.int32).numpy().astype(np.int64)
        mag = b & 0x7FFFFFFF
        return np.where(b < 0, -mag, mag)
    b = t.contiguous().view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    mag = b & 0x7FFF
    return np.where(b & 0x8000, -mag, mag)


def swiglu_case(T, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    gate = ((torch.rand(T, K, generator=g) * 2 - 1) * 88.0).to(dtype)
    up = torch.randn(T, K, generator=g).to(dtype)
    gate.view(-1)[:4] = torch.tensor([0.0, -0.0, 88.0, -88.0]).to(dtype)
    if T > 1:
        gate[1, :3] = torch.tensor([float("inf"), float("-inf"), float("nan")]).to(dtype)
        up[1, 3] = float("nan")
        up[1, 4] = float("inf")
    return gate, up


def silu64_product(gate, up):
    g, u = gate.double().numpy(), up.double().numpy()
    with np.errstate(all="ignore"):
        return g / (1.0 + np.exp(-g)), u


def ulp_distance(out: torch.Tensor, ref64: np.ndarray) -> np.ndarray:
    """Distance in ulps of the dtype between out and the (representable) float64 values ref64;
    NaN against NaN is 0, NaN against a number is huge."""
    ref = torch.from_numpy(ref64).to(out.dtype)
    assert np.array_equal(ref.double().numpy(), ref64, equal_nan=True)
    d = np.abs(order_key(out) - order_key(ref))
    n_out, n_ref = torch.isnan(out).numpy(), np.isnan(ref64)
    return np.where(n_out | n_ref, np.where(n_out & n_ref, 0, 1 << 40), d)


def run_swiglu(hip, gate, up, dev, strided=True, stats=True):
    T, K = gate.shape
    if strided:                                  # two column halves of one fused [T, 2K] buffer
        both = torch.cat([gate, up], dim=1).to(dev)
        gd, ud = both[:, :K], both[:, K:]
    else:
        gd, ud = gate.to(dev), up.to(dev)
    a = torch.zeros(K, dtype=torch.float64, device=dev) if stats else None
    s = torch.zeros(K, dtype=torch.float64, device=dev) if stats else None
    out = hip.swiglu_stats(gd, ud, 0, a, s)
    return out.cpu(), (finish(hip, a, s, T) if stats else None)


@pytest.mark.parametrize("K", (8, 264))
@pytest.mark.parametrize("dtype", (BF16, F16), ids=_ids)
def test_swiglu_within_one_ulp_and_exact_stats(dtype, K):
    dev, hip = _dev(), _hipmod()
    for T in (1, 300):
        gate, up = swiglu_case(T, K, dtype, 31 * K + T)
        s64, u64 = silu64_product(gate, up)
        with np.errstate(all="ignore"):
            ref = round64(round64(s64, dtype) * u64, dtype)
        for strided in (True, False):
            out, (m, q) = run_swiglu(hip, gate, up, dev, strided)
            d = ulp_distance(out, ref)
            print(f"swiglu {dtype} K={K} T={T} strided={strided}: max distance {int(d.max())} ulp, "
                  f"{int((d == 1).sum())} of {d.size} at 1 ulp")
            assert int(d.max()) <= 1
            ref_m, ref_s = orc.act_stats(out)
            assert same_bits(m, ref_m) and same_bits(q, ref_s)
        alone, _ = run_swiglu(hip, gate, up, dev, stats=False)
        assert same_values(alone, out)


# fp32: the bound is 4x the largest deviation from the float64 expression measured on the MI355X
# (2 ulp), capped at 16 ulp.
F32_SWIGLU_MEASURED_ULP = 2
F32_SWIGLU_BOUND_ULP = min(4 * F32_SWIGLU_MEASURED_ULP, 16)


@pytest.mark.parametrize("K", (8, 264))
def test_swiglu_fp32(K):
    dev, hip = _dev(), _hipmod()
    for T in (1, 300):
        gate, up = swiglu_case(T, K, F32, 31 * K + T)
        s64, u64 = silu64_product(gate, up)
        with np.errstate(all="ignore"):
            ref = (s64.astype(np.float32).astype(np.float64) * u64).astype(np.float32)
        out, (m, q) = run_swiglu(hip, gate, up, dev)
        d = np.abs(order_key(out) - order_key(torch.from_numpy(ref)))
        nan_o, nan_r = torch.isnan(out).numpy(), np.isnan(ref)
        assert np.array_equal(nan_o, nan_r)
        worst = int(d[~nan_r].max())
        print(f"swiglu fp32 K={K} T={T}: max distance {worst} ulp")
        assert worst <= F32_SWIGLU_BOUND_ULP
        ref_m, ref_s = orc.act_stats(out)
        assert same_bits(m, ref_m) and same_bits(q, ref_s)


# ---------------------------------------------------------------- guard bands
ESIZE = {BF16: 2, F16: 2, F32: 4}


class Guarded:
    """Buffers of one call in an arena; run() does both fill polarities and the three conditions of
    tests/test_gpu_bounds.py: nothing outside the outputs changes, every output byte is the
    expectation from any prior contents, with the workspace left holding the fill."""

    def __init__(self, dev):
        self.dev, self.specs = dev, []

    def inp(self, name, t, skew=0):
        self.specs.append(dict(name=name, data=t.detach().cpu().contiguous(), nbytes=t.numel() * t.element_size(),
                               skew=skew, untouched=True, expect=None))
        return len(self.specs) - 1

    def out(self, name, expect, skew=0, init=None):
        """init: contents stored before the call (an accumulator's zeros)."""
        e = expect.detach().cpu().contiguous()
        self.specs.append(dict(name=name, data=init, nbytes=e.numel() * e.element_size(), skew=skew, untouched=False,
                               expect=e))
        return len(self.specs) - 1

    def work(self, name, nbytes):
        self.specs.append(dict(name=name, data=None, nbytes=int(nbytes), skew=0, untouched=False, expect=None))
        return len(self.specs) - 1

    def run(self, launch):
        arena = Arena(Arena.required([s["nbytes"] for s in self.specs]), self.dev)
        regions = [arena.place(s["nbytes"], align=256, skew=s["skew"], name=s["name"], untouched=s["untouched"])
                   for s in self.specs]
        for complement in (False, True):
            arena.fill(3, complement)
            for s, r in zip(self.specs, regions):
                if s["data"] is not None:
                    r.store(s["data"])
            rc = launch([ctypes.c_void_p(r.data_ptr()) for r in regions])
            assert rc == 0, _hipmod().last_error()
            torch.cuda.synchronize(self.dev)
            arena.check()
            for s, r in zip(self.specs, regions):
                if s["expect"] is not None:
                    e = s["expect"]
                    got = r.load(e.dtype, e.shape)
                    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[e.element_size()]
                    ok = (got.view(it) == e.view(it)) | (torch.isnan(got) & torch.isnan(e))
                    assert bool(ok.all()), (s["name"], "complement" if complement else "plain")


def expected_sums(v: torch.Tensor):
    """fp64 running sums after one call of fewer than 256 rows... or any: the canonical order in
    numpy float64 (32-row sub-blocks, 256-row blocks, blocks onto the running value)."""
    x = v.double().numpy()
    T, K = x.shape
    with np.errstate(all="ignore"):
        acc = [np.zeros(K), np.zeros(K)]
        for b0 in range(0, T, 256):
            blk = [np.zeros(K), np.zeros(K)]
            for s0 in range(b0, min(b0 + 256, T), 32):
                sub = [np.zeros(K), np.zeros(K)]
                for t in range(s0, min(s0 + 32, b0 + 256, T)):
                    sub[0] = sub[0] + np.abs(x[t])
                    sub[1] = sub[1] + x[t] * x[t]
                blk = [blk[0] + sub[0], blk[1] + sub[1]]
            acc = [acc[0] + blk[0], acc[1] + blk[1]]
    return torch.from_numpy(acc[0]), torch.from_numpy(acc[1])


# (K, skew of the activations): the smallest shape on the 16-B path, the smallest on the fallback
GUARD_SHAPES = [(8, 0), (8, 2), (12, 0)]
GUARD_T = 270     # two blocks, the second partial


@pytest.mark.parametrize("K,skew", GUARD_SHAPES)
@pytest.mark.parametrize("dtype", (BF16, F32), ids=_ids)
def test_guard_accum(dtype, K, skew):
    dev, hip = _dev(), _hipmod()
    skew *= ESIZE[dtype] // 2
    x = rows(GUARD_T, K, dtype, 3)
    ea, es = expected_sums(x)
    m, s = orc.act_stats(x)
    assert same_bits((ea / GUARD_T).float(), m) and same_bits((es / GUARD_T).float(), s)   # the restatement above
    zero = torch.zeros(K, dtype=torch.float64)
    c = Guarded(dev)
    ix = c.inp("x", x, skew)
    iw = c.work("work", 8 * hip.calib_work_size(GUARD_T, K))
    ia, iq = c.out("acc_abs", ea, init=zero), c.out("acc_sq", es, init=zero)
    lib = hip.load_library()
    c.run(lambda p: lib.awq_act_stats_accum(p[ix], hip.AWQ_DTYPE[dtype], GUARD_T, K, K, 0, p[iw], p[ia], p[iq],
                                            _stream(dev)))


@pytest.mark.parametrize("K,skew", GUARD_SHAPES)
@pytest.mark.parametrize("dtype", (BF16, F32), ids=_ids)
def test_guard_rmsnorm(dtype, K, skew):
    dev, hip = _dev(), _hipmod()
    skew *= ESIZE[dtype] // 2
    x, w = norm_case(GUARD_T, K, dtype, 4)
    ref = rmsnorm_ref(x, w, 1e-5)
    ea, es = expected_sums(ref)
    zero = torch.zeros(K, dtype=torch.float64)
    c = Guarded(dev)
    ix, iwt = c.inp("x", x, skew), c.inp("weight", w)
    io = c.out("out", ref)
    iw = c.work("work", 8 * hip.calib_work_size(GUARD_T, K, norm=True))
    ia, iq = c.out("acc_abs", ea, init=zero), c.out("acc_sq", es, init=zero)
    lib = hip.load_library()
    c.run(lambda p: lib.awq_rmsnorm_stats(p[ix], hip.AWQ_DTYPE[dtype], GUARD_T, K, p[iwt], 1e-5, p[io], 0, p[iw],
                                          p[ia], p[iq], _stream(dev)))


@pytest.mark.parametrize("K,skew", GUARD_SHAPES)
@pytest.mark.parametrize("dtype", (BF16, F32), ids=_ids)
def test_guard_swiglu(dtype, K, skew):
    dev, hip = _dev(), _hipmod()
    skew *= ESIZE[dtype] // 2
    gate, up = swiglu_case(GUARD_T, K, dtype, 6)
    out, _ = run_swiglu(hip, gate, up, dev, strided=False)        # the kernel's own product (pinned above)
    ea, es = expected_sums(out)
    zero = torch.zeros(K, dtype=torch.float64)
    c = Guarded(dev)
    ig, iu = c.inp("gate", gate, skew), c.inp("up", up, skew)
    io = c.out("out", out)
    iw = c.work("work", 8 * hip.calib_work_size(GUARD_T, K))
    ia, iq = c.out("acc_abs", ea, init=zero), c.out("acc_sq", es, init=zero)
    lib = hip.load_library()
    c.run(lambda p: lib.awq_swiglu_stats(p[ig], p[iu], hip.AWQ_DTYPE[dtype], GUARD_T, K, K, p[io], 0, p[iw], p[ia],
                                         p[iq], _stream(dev)))
