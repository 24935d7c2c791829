"""awq_mxfp4_gemm on the GPU against tests/mxfp4_ref.py's dequantize of both operands and a
float64 matmul.

Exact case: scale bytes from {126, 127, 128}, so every product is a multiple of 2^-4 below 2^8 and every partial
sum over K <= 2048 is below 2^19: 23 bits, any summation order is exact in fp32, a wrong lane, nibble, block or
scale is a wrong bit.  General case (scale bytes in [100, 150]): |out - ref| <= K 2^-24 sum |a w| + 2^-24 |ref|,
the bound of any fp32 summation order; bf16 / fp16 outputs within one ulp of the rounded reference."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mxfp4_ref as ref
from guard_arena import Arena

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]
EXACT = [(1, 1, 32), (33, 65, 96), (130, 130, 320), (64, 256, 2048)]
BIASED = [(33, 65, 96), (130, 130, 320)]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
P = lambda r: ctypes.c_void_p(r.data_ptr())                # noqa: E731


def quantizer():
    from awq_quantizer.quantization.awq import AWQQuantizer
    return AWQQuantizer(bits=4, group_size=128, logger_level="ERROR")


@functools.lru_cache(maxsize=None)
def case(shape, lo, hi):
    """Random codes, scale bytes uniform in [lo, hi]: (a result, w result, bias fp32 [N], ref float64 [T, N],
    sum |a w| float64 [T, N]); results on the CPU, built once per shape."""
    T, N, K = shape
    rng = np.random.default_rng(T * 1009 + N * 31 + K + lo)
    ops = []
    for rows in (T, N):
        codes = rng.integers(0, 256, (rows, K // 2), dtype=np.uint8)
        scales = rng.integers(lo, hi + 1, (rows, K // 32), dtype=np.uint8)
        ops.append((codes, scales, ref.dequantize(codes, scales)))
    result = lambda c, s: {"codes": torch.from_numpy(c), "scales": torch.from_numpy(s), "format": "mxfp4",   # noqa: E731
                           "shape": torch.tensor([c.shape[0], K], dtype=torch.int64)}
    (ac, asc, a), (wc, ws, w) = ops
    bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
    return result(ac, asc), result(wc, ws), bias, a @ w.T, np.abs(a) @ np.abs(w).T


@pytest.mark.parametrize("shape", EXACT, ids=str)
def test_exact(shape):
    from awq_quantizer.quantization.mxfp4 import mxfp4_matmul
    a, w, _, want, _ = case(shape, 126, 128)
    got = mxfp4_matmul(quantizer(), a, w).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", BIASED, ids=str)
def test_general_with_bias(shape, dt):
    from awq_quantizer.quantization.mxfp4 import mxfp4_matmul
    a, w, bias, want, mass = case(shape, 100, 150)
    want = want + bias.double().numpy()
    bound = shape[2] * 2.0 ** -24 * (mass + np.abs(bias.numpy())) + 2.0 ** -24 * np.abs(want)
    got = mxfp4_matmul(quantizer(), a, w, bias, DTYPES[dt]).cpu()
    assert got.dtype == DTYPES[dt]
    if dt != "fp32":      # the fp32 result within the bound, then one rounding: one ulp of the rounded reference
        want = torch.from_numpy(want).to(DTYPES[dt]).double().numpy()
        bound = bound + 2.0 ** np.floor(np.log2(np.maximum(np.abs(want), 1e-300))) * torch.finfo(DTYPES[dt]).eps
    got = got.double().numpy()
    with np.errstate(invalid="ignore"):       # fp16: both beyond the type's range, the same infinity
        err = np.where(got == want, 0.0, np.abs(got - want))
        bound = np.where(np.isinf(want), 0.0, bound)
    print(f"{shape} {dt}: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
    assert (err <= bound).all()


def test_a_nan_scale_byte_marks_its_row_and_column():
    from awq_quantizer.quantization.mxfp4 import mxfp4_matmul
    a, w, _, _, _ = case((33, 65, 96), 100, 150)
    q = quantizer()
    clean = mxfp4_matmul(q, a, w).cpu()
    a2, w2 = dict(a, scales=a["scales"].clone()), dict(w, scales=w["scales"].clone())
    a2["scales"][2, 1], w2["scales"][5, 2] = 255, 255
    got = mxfp4_matmul(q, a2, w2).cpu()
    marked = torch.zeros(33, 65, dtype=torch.bool)
    marked[2, :], marked[:, 5] = True, True
    assert torch.equal(torch.isnan(got), marked)
    assert torch.equal(got[~marked].view(torch.int32), clean[~marked].view(torch.int32))


def test_guard_bands_and_dirty_buffers():
    from awq_quantizer import _hip
    lib = _hip.load_library()
    T, N, K = shape = (130, 130, 320)
    a, w, bias, want, _ = case(shape, 126, 128)
    want = (torch.from_numpy(want).float() + bias).numpy()      # exact sums, one fp32 addition
    sizes = [T * K // 2, T * K // 32, N * K // 2, N * K // 32, N * 4, T * N * 4]
    outs = []
    for complement in (False, True):
        arena = Arena(Arena.required(sizes), device="cuda")
        # the scale bytes at odd addresses; the codes keep the 16-B alignment the entry asks for
        names = (("a_codes", 0), ("a_scales", 1), ("w_codes", 16), ("w_scales", 3), ("bias", 4))
        regs = [arena.place(n, skew=k, name=name, untouched=True) for n, (name, k) in zip(sizes, names)]
        out = arena.place(sizes[5], skew=4, name="out", untouched=True)
        arena.fill(11, complement)
        for r, t in zip(regs, (a["codes"], a["scales"], w["codes"], w["scales"], bias)):
            r.store(t)
        assert lib.awq_mxfp4_gemm(P(regs[0]), P(regs[1]), T, P(regs[2]), P(regs[3]), N, 48, None, 0, P(out), 2, None) != 0
        arena.check()                                           # the refusal wrote nothing
        arena.mark_untouched(out, False)
        assert lib.awq_mxfp4_gemm(P(regs[0]), P(regs[1]), T, P(regs[2]), P(regs[3]), N, K, P(regs[4]), 2, P(out), 2,
                                  None) == 0, _hip.last_error()
        arena.check()
        outs.append(out.load(torch.float32, (T, N)).numpy())
    for got in outs:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_linear_is_quantize_then_matmul():
    from awq_quantizer.quantization.mxfp4 import mxfp4_matmul
    q = quantizer()
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(40, 320, generator=g) * 3).bfloat16()
    w = q.quantize_mxfp4((torch.randn(72, 320, generator=g) * 0.05).bfloat16(), "mse")
    bias = torch.randn(72, generator=g).bfloat16()
    got = q.mxfp4_linear(x, w, bias)
    want = mxfp4_matmul(q, q.quantize_mxfp4(x, "floor"), w, bias, torch.bfloat16)
    assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert q.mxfp4_linear(x, w, dtype=torch.float32, act_rule="ceil").dtype == torch.float32
    with pytest.raises(ValueError):
        q.mxfp4_linear(x[:, :288], w)


@pytest.mark.parametrize("rule", ["floor", "ceil", "mse"])
def test_requantizing_a_dequantized_weight_is_exact(rule):
    q = quantizer()
    w = (torch.randn(64, 256, generator=torch.Generator().manual_seed(5)) * 0.02).bfloat16()
    first = q.dequantize_mxfp4(q.quantize_mxfp4(w, rule), torch.bfloat16)
    again = q.dequantize_mxfp4(q.quantize_mxfp4(first, "floor"), torch.bfloat16)
    assert torch.equal(first.view(torch.int16), again.view(torch.int16))
