"""GPTQ's error-compensated rounding restated with NumPy on the CPU: what the tests compare
awq_gptq_round_block and AWQQuantizer.quantize_gptq against (include/awq_hip.h).

round_block is the kernel's definition in float32, one NumPy operation per rounded fp32 operation
(a product and the difference that uses it are two statements), the rows as a vector.  A group's
scale bits and zero point come from the unchanged CPU oracle on the group's fp32 slice as it
stands when the solver reaches its first column.  solve() adds the caller's part, the update of
the columns right of each block, and runs in float32 or float64 (dtype=): the float64 run is the
yardstick the fp32 loss is measured against, with the group rule written out in float64.
"""
import numpy as np
import torch

from oracle import awq_oracle as orc

BLOCK = 128
INT32_MIN = -2 ** 31


def inputs(N, K, T, seed):
    """The issue's seeded inputs: correlated samples X [T, K] and weights W [N, K], float64."""
    g = np.random.default_rng(seed)
    mix = g.standard_normal((K, K)) * (g.random((K, K)) < 0.05) + np.eye(K)
    X = (g.standard_normal((T, K)) * np.exp(g.standard_normal(K))) @ mix * 0.2
    W = 0.05 * g.standard_normal((N, K))
    return X, W


def factor(X, damp=0.01):
    """(U float64 upper with (H + damp mean(diag H) I)^-1 = U^T U, dead columns) for H = X^T X; a
    column with H[c][c] == 0 gets H[c][c] = 1."""
    X = np.asarray(X, dtype=np.float64)
    H = X.T @ X
    dead = np.diag(H) == 0
    H[dead, dead] = 1.0
    H[np.diag_indices_from(H)] += damp * np.mean(np.diag(H))
    Hinv = np.linalg.inv(H)
    Hinv = (Hinv + Hinv.T) / 2
    return np.linalg.cholesky(Hinv).T.copy(), dead


def qrange(bits, sym):
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if sym else (0, (1 << bits) - 1)


def group_params32(seg, bits, sym):
    """The project's fp32 rule on the groups seg [N, gs] (float32): (fp16 scale bits uint16 [N],
    zero points int64 [N], INT32_MIN for a NaN one), from the oracle."""
    N, gs = seg.shape
    _, sc, zp = orc.quantize_groups(torch.from_numpy(np.ascontiguousarray(seg)), N, gs, gs, bits, sym)
    return sc.view(torch.int16).numpy().reshape(N).astype(np.uint16), zp.numpy().reshape(N).astype(np.int64)


def group_params64(seg, bits, sym):
    """The same rule in float64 arithmetic (finite groups): (fp16 scale bits, zero points)."""
    qr = float((1 << bits) - 1)
    mn, mx = seg.min(axis=1), seg.max(axis=1)
    if sym:
        a = np.maximum(np.abs(mn), np.abs(mx))
        mn, mx = -a, a
    s = np.maximum((mx - mn) / qr, 1e-10)
    z = np.zeros_like(s) if sym else np.clip(np.rint(-(mn / s)), 0.0, qr)
    return s.astype(np.float16).view(np.uint16), z.astype(np.int64)


def round_block(work, U, gs, bits, sym, c0, n, fields, zfields, sbits, propagate=True):
    """Columns [c0, c0 + n) of work [N, K] (float32 or float64, updated in place) against the upper
    factor U [K, K] of work's dtype.  Writes the block's fields [N, K], zero fields [N, G] and scale
    bits [N, G] (uint16); -> err [N, n].  propagate=False: round to nearest with the same rule."""
    dt = work.dtype
    f32 = dt == np.float32
    N = work.shape[0]
    qmin, qmax = qrange(bits, sym)
    mask = (1 << bits) - 1
    err = np.zeros((N, n), dtype=dt)
    s = z = None
    with np.errstate(all="ignore"):
        for i in range(n):
            c = c0 + i
            if i % gs == 0:
                seg = work[:, c:c + gs]
                hb, zp = group_params32(seg, bits, sym) if f32 else group_params64(seg, bits, sym)
                g = c // gs
                sbits[:, g] = hb
                zfields[:, g] = np.where(zp == INT32_MIN, -qmin, zp - qmin) & mask
                s = hb.view(np.float16).astype(dt)
                z = np.where(zp == INT32_MIN, np.nan, zp).astype(dt)
            w = work[:, c].copy()
            quo = w / s
            r = np.rint(quo) + z
            rnan = np.isnan(r)
            qf = np.minimum(np.maximum(np.where(rnan, dt.type(qmin), r), dt.type(qmin)), dt.type(qmax))
            fields[:, c] = np.where(rnan, (-qmin) & mask, qf.astype(np.int64) - qmin)
            dq = (qf - z) * s
            dq = np.where(rnan, r, dq)
            d = w - dq
            e = d / U[c, c]
            e = np.where(np.isfinite(s) & np.isfinite(dq) & np.isfinite(quo), e, dt.type(0)).astype(dt)
            err[:, i] = e
            if propagate and i + 1 < n:
                p = e[:, None] * U[c, c + 1:c0 + n][None, :]          # RN(e u)
                work[:, c + 1:c0 + n] = work[:, c + 1:c0 + n] - p      # RN(w - RN(e u))
    return err


def solve(W, U, gs, bits, sym, dtype=np.float32, propagate=True, dead=None):
    """The whole solver on W [N, K]: blocks of 128 columns, then the update of the columns to the
    right (a GEMM: its summation order is the library's, so a float32 run is compared through its
    loss, not bit for bit).  -> {"fields", "zfields", "sbits", "work"}."""
    work = np.array(W, dtype=dtype)
    if dead is not None:
        work[:, dead] = 0
    U = np.asarray(U, dtype=dtype)
    N, K = work.shape
    out = {"fields": np.zeros((N, K), np.int64), "zfields": np.zeros((N, K // gs), np.int64),
           "sbits": np.zeros((N, K // gs), np.uint16), "work": work}
    for c0 in range(0, K, BLOCK):
        c1 = min(c0 + BLOCK, K)
        err = round_block(work, U, gs, bits, sym, c0, c1 - c0, out["fields"], out["zfields"], out["sbits"], propagate)
        if propagate and c1 < K:
            work[:, c1:] = work[:, c1:] - err @ U[c0:c1, c1:]
    return out


def dequantize(res, gs):
    """(field - zero field) * fp16 scale in float64 [N, K] (exact: a small integer times an fp16)."""
    s = res["sbits"].view(np.float16).astype(np.float64)
    return (res["fields"] - np.repeat(res["zfields"], gs, axis=1)).astype(np.float64) * np.repeat(s, gs, axis=1)


def output_loss(Wq, W, X):
    """sum ((Wq - W) X^T)^2 in float64."""
    E = (np.asarray(Wq, np.float64) - np.asarray(W, np.float64)) @ np.asarray(X, np.float64).T
    return float((E * E).sum())


def pack_words(fields, bits):
    """int fields [R, n] -> int32 words [R, ceil(n bits / 32)], field j of a word at bits [bits j, +bits)."""
    per = 32 // bits
    R, n = fields.shape
    Wn = -(-n // per)
    f = np.zeros((R, Wn * per), np.int64)
    f[:, :n] = fields & ((1 << bits) - 1)
    f = f.reshape(R, Wn, per)
    w = np.zeros((R, Wn), np.int64)
    for j in range(per):
        w |= f[:, :, j] << (bits * j)
    return w.astype(np.uint32).view(np.int32)
