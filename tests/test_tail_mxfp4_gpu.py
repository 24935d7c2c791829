"""MXFP4 on the GPU: awq_quantize_mxfp4 / awq_dequantize_mxfp4 / awq_mxfp4_error through
AWQQuantizer, bit for bit against the float64 restatement of the format in tests/mxfp4_ref.py.

"mse": the kernel's two error sums are fp32, so blocks whose float64 candidate errors differ by less than
1e-5 relative are left out of the comparison (at most 0.1 % of a case's blocks); an all-zero block is a
tie by construction, is not left out, and must come out as the floor candidate.
Error report: the sums against float64 sums at rel 1e-5, tests/test_gpu_qerror.py's tolerance for them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mxfp4_ref as ref
from guard_arena import Arena

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
SHAPES = [(1, 32), (3, 96), (5, 2080), (64, 4096)]
RULES = ["floor", "ceil", "mse"]


def crafted_blocks(dtype, rng):
    """The blocks of 32 written over the first blocks of a case (float64, exact in dtype)."""
    k, X = -3, -5
    body = lambda top: rng.uniform(-0.9, 0.9, 32) * top          # noqa: E731
    out = [np.zeros(32), -np.zeros(32)]
    for special in (np.nan, -np.inf):
        b = body(0.02)
        b[7] = special
        out.append(b)
    for m in (1.0, 6.0, 7.0, 7.5):
        b = body(2.0 ** k)
        b[5] = -m * 2.0 ** k
        out.append(b)
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    b = np.full(32, 0.5)        # the rest on the floor candidate's grid only: no near tie under "mse"
    b[0], b[1:8], b[8:15] = 4.0, ties, -ties
    out.append(b * 2.0 ** X)
    b = body(1.0)
    b[31] = float(torch.finfo(dtype).max)
    out.append(b)
    if dtype != torch.float16:
        b = np.zeros(32)
        b[:6] = [2.0 ** -126, -2.0 ** -127, 3 * 2.0 ** -128, 2.0 ** -128, 2.0 ** -129, 3 * 2.0 ** -129]
        out.append(b)
    if dtype == torch.float32:
        b = body(2.0 ** 126)
        b[3] = 1.5 * 2.0 ** 127
        out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def case(dt, shape):
    """(the weight on the CPU in dtype, the same as float64 NumPy), built once per dtype and shape."""
    rng = np.random.default_rng(shape[0] * 7919 + shape[1])
    x = rng.standard_normal(shape) * 0.02
    blocks = x.reshape(-1, 32)
    for i, b in enumerate(crafted_blocks(DTYPES[dt], rng)[:blocks.shape[0]]):
        blocks[i] = b
    t = torch.from_numpy(x).to(DTYPES[dt])
    return t, t.double().numpy()


@functools.lru_cache(maxsize=None)
def expected(dt, shape, rule):
    return ref.quantize(case(dt, shape)[1], rule)


def quantizer():
    from awq_quantizer.quantization.awq import AWQQuantizer
    return AWQQuantizer(bits=4, group_size=128, logger_level="ERROR")


def compare(result, dt, shape, rule):
    codes, scales, near = expected(dt, shape, rule)
    got_c, got_s = result["codes"].cpu().numpy(), result["scales"].cpu().numpy()
    assert got_c.dtype == np.uint8 and got_c.shape == codes.shape and got_s.shape == scales.shape
    print(f"{dt} {shape} {rule}: {near.sum()} of {near.size} blocks left out")
    assert near.mean() <= 1e-3
    keep = ~near
    assert np.array_equal(got_s[keep], scales[keep])
    g, w = ref.nibbles(got_c), ref.nibbles(codes)
    same = (g == w) | (((g | w) & 7) == 0)                      # a zero magnitude matches whatever its sign
    assert same[np.repeat(keep, 32, axis=1)].all()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dt", DTYPES)
def test_quantize(dt, rule, shape):
    r = quantizer().quantize_mxfp4(case(dt, shape)[0], rule)
    assert r["format"] == "mxfp4" and r["scale_rule"] == rule and r["shape"].tolist() == list(shape)
    assert r["codes"].is_cuda and r["scales"].is_cuda
    compare(r, dt, shape, rule)


@pytest.mark.parametrize("dt,rule", [("bf16", "mse"), ("fp32", "floor")])
def test_quantize_later_trips(dt, rule):
    """A grid of 2 workgroups: the 6 segments of (5, 2080) take three trips each."""
    from awq_quantizer import _hip
    q, shape = quantizer(), (5, 2080)
    with _hip.tuning(max_blocks=2):
        r = q.quantize_mxfp4(case(dt, shape)[0], rule)
        back = q.dequantize_mxfp4(r)
        err = q.quantization_error(case(dt, shape)[0], r)
    compare(r, dt, shape, rule)
    assert torch.equal(back.cpu().nan_to_num(nan=7.0), q.dequantize_mxfp4(r).cpu().nan_to_num(nan=7.0))
    assert err == q.quantization_error(case(dt, shape)[0], r)


def synthetic(shape):
    """Every code against scale bytes that include both ends, the NaN byte and the overflow range."""
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 256, (shape[0], shape[1] // 2), dtype=np.uint8)
    scales = rng.integers(0, 256, (shape[0], shape[1] // 32), dtype=np.uint8)
    edge = np.array([0, 1, 2, 14, 103, 126, 127, 128, 142, 143, 144, 252, 253, 254, 255], dtype=np.uint8)
    scales.reshape(-1)[:min(edge.size, scales.size)] = edge[:scales.size]
    return codes, scales


@pytest.mark.parametrize("shape", [(1, 32), (5, 2080)], ids=str)
@pytest.mark.parametrize("dt", DTYPES)
def test_dequantize(dt, shape):
    codes, scales = synthetic(shape)
    result = {"codes": torch.from_numpy(codes), "scales": torch.from_numpy(scales), "format": "mxfp4",
              "shape": torch.tensor(shape)}
    got = quantizer().dequantize_mxfp4(result, DTYPES[dt]).cpu()
    with np.errstate(over="ignore"):
        want = torch.from_numpy(ref.dequantize(codes, scales)).to(DTYPES[dt])      # exact in fp32, then one rounding
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got.isnan(), want.isnan())
    view = torch.int32 if dt == "fp32" else torch.int16
    assert torch.equal(got.nan_to_num(nan=0.0).view(view), want.nan_to_num(nan=0.0).view(view))


@pytest.mark.parametrize("shape", [(3, 96), (5, 2080), (64, 4096)], ids=str)
@pytest.mark.parametrize("dt", DTYPES)
def test_error_report(dt, shape):
    t, x = case(dt, shape)
    q = quantizer()
    r = q.quantize_mxfp4(t, "floor")
    got = q.quantization_error(t, r)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - ref.dequantize(r["codes"].cpu().numpy(), r["scales"].cpu().numpy())
        d32, x32 = d.astype(np.float32), x.astype(np.float32)
        fin = np.isfinite(d32 * d32) & np.isfinite(x32 * x32)                   # the report's fp32 test
    d, w = np.where(fin, d, 0.0), np.where(fin, x, 0.0)
    want = {"sum_abs": np.abs(d).sum(), "sum_sq": (d * d).sum(), "sum_w_sq": (w * w).sum(),
            "max_abs_error": np.abs(d).max()}
    print(dt, shape, {k: (got[k], float(v)) for k, v in want.items()}, got["nonfinite"], int((~fin).sum()))
    assert got["numel"] == x.size and got["nonfinite"] == int((~fin).sum()) and got["input_scaled"] is False
    for k, v in want.items():
        assert got[k] == pytest.approx(float(v), rel=1e-5), k
    with pytest.raises(ValueError):
        q.quantization_error(t, r, per_group=True)
    with pytest.raises(ValueError):
        q.quantization_error(t, r, samples=torch.zeros(2, shape[1]))


def test_k_48_is_refused_and_nothing_is_written():
    from awq_quantizer import _hip
    lib = _hip.load_library()
    rows, K = 4, 48
    arena = Arena(Arena.required([rows * K * 2, rows * K // 2, rows * 2, 4096]), device="cuda")
    x = arena.place(rows * K * 2, name="x")
    codes = arena.place(rows * K // 2, name="codes", untouched=True)
    scales = arena.place(rows * 2, name="scales", untouched=True)
    out = arena.place(4096, name="out", untouched=True)
    arena.fill(3)
    P = lambda r: ctypes.c_void_p(r.data_ptr())                # noqa: E731
    assert lib.awq_quantize_mxfp4(P(x), 0, rows, K, 0, P(codes), P(scales), None) != 0
    assert "K % 32" in _hip.last_error()
    assert lib.awq_dequantize_mxfp4(P(codes), P(scales), rows, K, 0, P(out), None) != 0
    assert lib.awq_mxfp4_error(P(x), 0, P(codes), P(scales), rows, K, P(out), None) != 0
    assert lib.awq_quantize_mxfp4(P(x), 3, rows, 64, 0, P(codes), P(scales), None) != 0      # fp64
    assert lib.awq_quantize_mxfp4(P(x), 0, rows, 64, 3, P(codes), P(scales), None) != 0      # the rule
    assert lib.awq_quantize_mxfp4(P(x), 0, rows, 64, 0, None, P(scales), None) != 0
    arena.check()
