"""MXFP4 restated in float64 NumPy from the format's definition: the reference of
tests/test_tail_mxfp4_gpu.py and the independent reader of tests/test_tail_mxfp4_model_gpu.py."""
import numpy as np

MAGS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
MIDS = (MAGS[:-1] + MAGS[1:]) / 2                      # 0.25 0.75 1.25 1.75 2.5 3.5 5
TIE_UP = np.arange(7) % 2 == 1                         # a tie between indices i, i + 1 goes to the even one


def _encode(b, X):
    """Blocks b [..., 32] at the exponents X [...]: (magnitude index, dequantized float64)."""
    v = np.ldexp(np.abs(b), -X[..., None])             # exact
    idx = (v[..., None] > MIDS).sum(-1) + ((v[..., None] == MIDS) & TIE_UP).sum(-1)
    return idx, np.copysign(np.ldexp(MAGS[idx], X[..., None]), b)


def quantize(x, rule):
    """x float64 [N, K] -> (codes uint8 [N, K / 2], scales uint8 [N, K / 32], near_tie bool [N, K / 32]:
    blocks whose two "mse" candidates' errors differ by less than 1e-5 relative)."""
    N, K = x.shape
    b = x.reshape(N, K // 32, 32)
    bad = ~np.isfinite(b).all(-1)
    b = np.where(bad[..., None], 0.0, b)
    amax = np.abs(b).max(-1)
    X0 = np.where(amax == 0, 0, np.clip(np.frexp(amax)[1] - 1 - 2, -127, 127)).astype(np.int64)
    X1 = np.minimum(X0 + 1, 127)
    (i0, d0), (i1, d1) = _encode(b, X0), _encode(b, X1)
    e0, e1 = ((b - d0) ** 2).sum(-1), ((b - d1) ** 2).sum(-1)
    up = {"floor": np.zeros_like(bad), "ceil": np.ldexp(amax, -X0) > 6, "mse": e1 < e0}[rule]
    near = (np.abs(e0 - e1) < 1e-5 * np.maximum(e0, e1)) & ~bad if rule == "mse" else np.zeros_like(bad)
    idx = np.where(up[..., None], i1, i0) | (np.signbit(b) << 3)
    idx = np.where(bad[..., None], 0, idx).reshape(N, K).astype(np.uint8)
    scales = np.where(bad, 255, np.where(up, X1, X0) + 127).astype(np.uint8)
    return idx[:, 0::2] | (idx[:, 1::2] << 4), scales, near


def nibbles(codes):
    """codes uint8 [N, K / 2] -> the 4-bit codes [N, K]."""
    return np.stack([codes & 15, codes >> 4], axis=-1).reshape(codes.shape[0], -1)


def dequantize(codes, scales):
    """-> float64 [N, K]: +-mag 2^(e - 127); a block whose scale byte is 255 is NaN."""
    c = nibbles(codes).astype(np.int64)
    e = np.repeat(scales.astype(np.int64), 32, axis=1)
    v = np.ldexp(np.where(c & 8, -MAGS[c & 7], MAGS[c & 7]), e - 127)
    return np.where(e == 255, np.nan, v)
