"""GPTQ-compensated MXFP4 restated with NumPy on the CPU: what the tests compare
awq_gptq_round_block_mxfp4 and AWQQuantizer.quantize_gptq_mxfp4 against (include/awq_hip.h;
DESIGN.md §5.23).

round_block is the kernel's definition in float32, one NumPy statement per rounded fp32 operation
(a product and the difference that uses it are two statements), the rows as a vector.  solve() adds
the caller's part, the update of the columns right of each call, and runs in float32 or float64
(dtype=): the float64 run is the yardstick the fp32 loss is measured against.
"""
import numpy as np

BLOCK = 128
RULES = {"floor": 0, "ceil": 1, "mse": 2}


def _round(a, inv, dt):
    """|x| = a at the scale inv = 2^-X: (magnitude index, rounded magnitude m, t = a 2^-X).  The ONE
    addition: 2^(22 + k) in float32 (ulp = the grid's step at v), 2^(51 + k) in float64."""
    t = a * inv
    v = np.fmin(t, dt.type(6))
    k = np.maximum(np.frexp(v)[1] - 1, 0)                                     # max(exponent of v, 0): 0, 1, 2
    magic = np.ldexp(dt.type(1), k + (22 if dt == np.float32 else 51)).astype(dt)
    r = v + magic
    m = r - magic
    idx = np.select([m < 2, m < 4], [m * 2, m + 2], m / 2 + 4).astype(np.int64)
    return idx, m, t


def _sq_error(seg, inv, dt):
    """sum (t - m)^2 over the blocks seg [N, 32]: four runs of 8 in order from +0, (p0 + p1) + (p2 + p3)."""
    _, m, t = _round(np.abs(seg), inv[:, None], dt)
    d = t - m
    sq = d * d
    p = []
    for r in range(4):
        s = np.zeros(seg.shape[0], dt)
        for i in range(8):
            s = s + sq[:, 8 * r + i]
        p.append(s)
    return (p[0] + p[1]) + (p[2] + p[3])


def block_scale(seg, rule, dt):
    """The blocks seg [N, 32] as they stand -> (scale byte int64 [N], bad [N], inv = 2^-X, scale = 2^X)."""
    bad = ~np.isfinite(seg).all(axis=1)
    amax = np.abs(np.where(bad[:, None], dt.type(0), seg)).max(axis=1)
    E = np.where(amax == 0, 0, np.frexp(amax)[1] - 1 + 127)                     # the biased fp32 exponent
    e = np.where(amax == 0, 127, np.maximum(np.maximum(E, 0), 2) - 2).astype(np.int64)
    inv = np.ldexp(dt.type(1), 127 - e).astype(dt)
    if rule == "mse":
        up = dt.type(4) * _sq_error(seg, inv * dt.type(0.5), dt) < _sq_error(seg, inv, dt)
    elif rule == "ceil":
        up = amax * inv > dt.type(6)
    else:
        up = np.zeros(seg.shape[0], bool)
    up &= ~bad
    e = e + up
    inv = np.where(up, inv * dt.type(0.5), inv)
    return np.where(bad, 255, e), bad, inv, np.ldexp(dt.type(1), e - 127).astype(dt)


def round_block(work, U, rule, c0, n, idx, sbytes, propagate=True):
    """Columns [c0, c0 + n) of work [N, K] (float32 or float64, updated in place) against the upper
    factor U [K, K] of work's dtype.  Writes the call's 4-bit codes idx [N, K] and scale bytes
    sbytes [N, K / 32]; -> err [N, n].  propagate=False: round to nearest with the same rule."""
    dt = work.dtype
    N = work.shape[0]
    err = np.zeros((N, n), dtype=dt)
    with np.errstate(all="ignore"):
        for i in range(n):
            c = c0 + i
            if i % 32 == 0:
                sbytes[:, c // 32], bad, inv, scale = block_scale(work[:, c:c + 32], rule, dt)
            w = work[:, c].copy()
            mag, m, _ = _round(np.abs(w), inv, dt)
            dq = np.copysign(m * scale, w)
            d = w - dq
            e = d / U[c, c]
            e = np.where(np.isfinite(w) & np.isfinite(dq) & np.isfinite(e) & ~bad, e, dt.type(0)).astype(dt)
            idx[:, c] = np.where(bad, 0, mag | (np.signbit(w).astype(np.int64) << 3))
            err[:, i] = e
            if propagate and i + 1 < n:
                p = e[:, None] * U[c, c + 1:c0 + n][None, :]          # RN(e u)
                work[:, c + 1:c0 + n] = work[:, c + 1:c0 + n] - p      # RN(w - RN(e u))
    return err


def solve(W, U, rule, dtype=np.float32, propagate=True, dead=None):
    """The whole solver on W [N, K]: calls of 128 columns, then the update of the columns to the right
    (a GEMM: its summation order is the library's, so a float32 run is compared through its loss,
    not bit for bit).  -> {"idx", "sbytes", "work"}."""
    work = np.array(W, dtype=dtype)
    if dead is not None:
        work[:, dead] = 0
    U = np.asarray(U, dtype=dtype)
    N, K = work.shape
    out = {"idx": np.zeros((N, K), np.int64), "sbytes": np.zeros((N, K // 32), np.int64), "work": work}
    for c0 in range(0, K, BLOCK):
        c1 = min(c0 + BLOCK, K)
        err = round_block(work, U, rule, c0, c1 - c0, out["idx"], out["sbytes"], propagate)
        if propagate and c1 < K:
            work[:, c1:] = work[:, c1:] - err @ U[c0:c1, c1:]
    return out


def pack(idx):
    """4-bit codes [N, K] -> uint8 [N, K / 2], the even element in the low nibble."""
    idx = idx.astype(np.uint8)
    return idx[:, 0::2] | (idx[:, 1::2] << 4)
