"""Activation-aware MXFP4 on the GPU: awq_quantize_mxfp4_scaled byte for byte against the
two entries it fuses, awq_act_search_losses_mxfp4 bit for bit against a NumPy float32 restatement (one
statement per rounded operation; the block's byte and codes from tests/mxfp4_ref.py), the selection, the
Python methods, the refusals and the stream.

"mse": a (candidate, block) pair whose float64 candidate errors are within 1e-5 relative is left out, at
most 0.1 % of a case's pairs; the cap is asserted on the reference before the GPU runs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mxfp4_ref as ref
import stream_gate
from guard_arena import Arena
from test_tail_mxfp4_gpu import DTYPES, RULES, SHAPES, case, quantizer

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]
RULE_CODE = {"floor": 0, "ceil": 1, "mse": 2}
# n_grid 33: one past the 32 candidates the loss kernel stages in LDS at once
LOSS_CASES = [(s, n) for s in SHAPES for n in (1, 5)] + [((64, 4096), 20), ((3, 96), 33)]
P = lambda r: ctypes.c_void_p(r.data_ptr())                # noqa: E731


@functools.lru_cache(maxsize=None)
def table_of(K, n_grid):
    """awq_act_scale_table on random statistics (CPU copy).  Grids of 5 and more also carry, in the last
    two candidates, a block of entries outside [2^-60, 2^60] each (their reciprocals are NaN: the IEEE path);
    whole blocks, since one such column alone would dominate its block and tie the two "mse" candidates."""
    from awq_quantizer import _hip
    g = torch.Generator().manual_seed(K + n_grid)
    x_mean = (torch.rand(K, generator=g) * 4 + 0.01).cuda()
    t = _hip.act_scale_table(x_mean, None, n_grid).cpu()
    if n_grid >= 5:
        t[-1, :32], t[-2, K - 32:] = 2.0 ** 70, 2.0 ** -70
    return t


@functools.lru_cache(maxsize=None)
def x_sq_of(K):
    return torch.rand(K, generator=torch.Generator().manual_seed(K)) * 3 + 0.1


def col_scales(K):
    s = torch.ones(K)
    s[1::7], s[3::11] = 2.0 ** -20, 2.0 ** 20
    return {"table": table_of(K, 5)[2].clone(), "ones": torch.ones(K), "extreme": s}


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dt", DTYPES)
def test_quantize_scaled(dt, rule, shape):
    from awq_quantizer import _hip
    lib = _hip.load_library()
    w, (N, K) = case(dt, shape)[0], shape
    q = quantizer()
    for name, s in col_scales(K).items():
        arena = Arena(Arena.required([w.numel() * w.element_size(), K * 4, N * K // 2, N * K // 32]), device="cuda")
        rw = arena.place(w.numel() * w.element_size(), name="w", untouched=True)
        rs = arena.place(K * 4, name="col_scale", untouched=True)
        rc, re = arena.place(N * K // 2, name="codes"), arena.place(N * K // 32, name="scales")
        arena.fill(5)
        rw.store(w)
        rs.store(s)
        assert lib.awq_quantize_mxfp4_scaled(P(rw), _hip.AWQ_DTYPE[w.dtype], N, K, RULE_CODE[rule], P(rs), P(rc), P(re),
                                             None) == 0, _hip.last_error()
        arena.check()
        got_c, got_s = rc.load(torch.uint8, (N, K // 2)), re.load(torch.uint8, (N, K // 32))
        two = q.quantize_mxfp4(_hip.apply_input_scale(w.cuda(), s.cuda()), rule)
        assert torch.equal(got_c, two["codes"].cpu()) and torch.equal(got_s, two["scales"].cpu()), name
        if rule == "floor":
            codes, scales, _ = ref.quantize((w.float() * s).to(w.dtype).double().numpy(), rule)
            assert np.array_equal(got_s.numpy(), scales), name
            g, e = ref.nibbles(got_c.numpy()), ref.nibbles(codes)
            assert ((g == e) | (((g | e) & 7) == 0)).all(), name   # a zero magnitude matches whatever its sign


@functools.lru_cache(maxsize=None)
def expected_losses(dt, shape, rule, n_grid):
    """(part float32 [n_grid, N K / 32], near bool of the same shape) of the reference."""
    w, (N, K) = case(dt, shape)[0], shape
    table, x_sq = table_of(K, n_grid), x_sq_of(K).numpy()
    w32 = w.float().numpy()
    part = np.empty((n_grid, N * K // 32), dtype=np.float32)
    near = np.empty(part.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(n_grid):
            s = table[i]
            wp = (w.float() * s).to(w.dtype)                                  # RN_D(w s), torch CPU
            codes, scales, nr = ref.quantize(wp.double().numpy(), rule)
            dq = ref.dequantize(codes, scales).astype(np.float32)             # exact (beyond the range inf)
            quot = dq / s.numpy()
            d = quot - w32
            dd = d * d
            c = (x_sq * dd).reshape(N * K // 32, 4, 8)
            run = np.zeros(c.shape[:2], dtype=np.float32)
            for j in range(8):
                run = run + c[..., j]
            part[i] = (run[:, 0] + run[:, 1]) + (run[:, 2] + run[:, 3])
            near[i] = nr.reshape(-1)
    return part, near


@pytest.mark.parametrize("shape,n_grid", LOSS_CASES, ids=str)
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dt", DTYPES)
def test_losses(dt, rule, shape, n_grid):
    from awq_quantizer import _hip
    lib = _hip.load_library()
    w, (N, K) = case(dt, shape)[0], shape
    want, near = expected_losses(dt, shape, rule, n_grid)
    print(f"{dt} {shape} {rule} n_grid {n_grid}: {near.sum()} of {near.size} pairs left out")
    assert near.mean() <= 1e-3                                 # on the reference, before the GPU runs
    table, x_sq = table_of(K, n_grid), x_sq_of(K)
    rtable = _hip.act_recip_table(table.cuda()).cpu()
    nblk = N * K // 32
    for use_rt in (True, False):
        arena = Arena(Arena.required([w.numel() * w.element_size(), n_grid * K * 4, n_grid * K * 4, K * 4,
                                      n_grid * nblk * 4]), device="cuda")
        rw = arena.place(w.numel() * w.element_size(), name="w", untouched=True)
        rt, rr = arena.place(n_grid * K * 4, name="table", untouched=True), arena.place(n_grid * K * 4, name="rtable",
                                                                                       untouched=True)
        rx, rp = arena.place(K * 4, name="x_sq", untouched=True), arena.place(n_grid * nblk * 4, name="part")
        arena.fill(7)
        for r, t in ((rw, w), (rt, table), (rr, rtable), (rx, x_sq)):
            r.store(t)
        assert lib.awq_act_search_losses_mxfp4(P(rw), _hip.AWQ_DTYPE[w.dtype], N, K, RULE_CODE[rule], P(rt),
                                               P(rr) if use_rt else None, n_grid, P(rx), P(rp), nblk, None) == 0, \
            _hip.last_error()
        arena.check()
        got = rp.load(torch.float32, (n_grid, nblk)).numpy()
        keep = ~near
        assert np.array_equal(np.isnan(got)[keep], np.isnan(want)[keep])
        fin = keep & ~np.isnan(want)
        assert np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin]), f"rtable {use_rt}"
    # the selection, on the blocks behind the crafted ones (their NaN blocks make every candidate NaN): the
    # first minimum of the float64 sums of these partials (bit-equal to the reference's outside the left-out pairs)
    first = 16 if nblk > 16 else 0
    sub = torch.from_numpy(got[:, first:]).contiguous().cuda()
    _, best, s_best = _hip.act_search_select(sub, table.cuda())
    with np.errstate(all="ignore"):
        sums = got[:, first:].astype(np.float64).sum(1)
    order = np.where(np.isnan(sums), np.inf, sums)
    expect = int(order.argmin()) if not np.isnan(sums).all() else 0
    assert int(best.item()) == expect and torch.equal(s_best.cpu(), table[expect])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_layer_group(seed):
    from awq_quantizer import _hip
    g = torch.Generator().manual_seed(seed)
    K = 256
    weights = {"a": (torch.randn(8, K, generator=g) * 0.02).bfloat16(), "b": (torch.randn(24, K, generator=g) * 0.02).bfloat16()}
    acts = (torch.randn(64, K, generator=g) * (torch.rand(K, generator=g) * 4)).bfloat16()
    q = quantizer()
    out = q.quantize_layer_group_mxfp4(weights, acts, scale_rule="mse")
    losses = out["losses"].cpu()
    assert losses[out["best"]] == losses.min() and out["ratio"] == out["best"] / q.search_grid
    for name, w in weights.items():
        two = q.quantize_mxfp4(_hip.apply_input_scale(w.cuda(), out["input_scale"]), "mse")
        r = out["results"][name]
        assert torch.equal(r["codes"], two["codes"]) and torch.equal(r["scales"], two["scales"])
        assert r["format"] == "mxfp4" and torch.equal(r["input_scale"], out["input_scale"])
    ones = q.quantize_layer_group_mxfp4(weights, acts, table=torch.ones(q.search_grid, K))
    for name, w in weights.items():
        plain = q.quantize_mxfp4(w)
        assert torch.equal(ones["results"][name]["codes"], plain["codes"])
        assert torch.equal(ones["results"][name]["scales"], plain["scales"])


def test_refusals_write_nothing():
    from awq_quantizer import _hip
    lib = _hip.load_library()
    rows = 4
    arena = Arena(Arena.required([rows * 64 * 2, 4096, 4096, 4096]), device="cuda")
    x = arena.place(rows * 64 * 2, name="x")
    t = arena.place(4096, name="table")
    codes, part = arena.place(4096, name="codes", untouched=True), arena.place(4096, name="part", untouched=True)
    arena.fill(3)
    loss = lambda dt=0, K=64, rule=0, n=2, w=x, p=part: lib.awq_act_search_losses_mxfp4(   # noqa: E731
        P(w) if w else None, dt, rows, K, rule, P(t), None, n, P(t), P(p) if p else None, rows * 2, None)
    quant = lambda dt=0, K=64, rule=0, s=t: lib.awq_quantize_mxfp4_scaled(                    # noqa: E731
        P(x), dt, rows, K, rule, P(s) if s else None, P(codes), P(part), None)
    assert loss(K=48) != 0 and "K % 32" in _hip.last_error()
    assert quant(K=48) != 0 and "K % 32" in _hip.last_error()
    assert loss(dt=3) != 0 and quant(dt=3) != 0                     # fp64
    assert loss(rule=7) != 0 and quant(rule=7) != 0
    assert loss(n=0) != 0 and loss(n=_hip.ACT_MAX_GRID + 1) != 0 and "n_grid" in _hip.last_error()
    assert loss(w=None) != 0 and loss(p=None) != 0 and quant(s=None) != 0
    arena.check()


def test_off_the_default_stream():
    from awq_quantizer import _hip
    dev = torch.device("cuda")
    dt, shape, rule = "bf16", (5, 2080), "mse"
    (N, K), n_grid = shape, 5

    def make():
        w, table, x_sq = case(dt, shape)[0].cuda(), table_of(K, n_grid).cuda(), x_sq_of(K).cuda()
        rtable = _hip.act_recip_table(table)
        codes = torch.zeros((N, K // 2), dtype=torch.uint8, device=dev)
        scales = torch.zeros((N, K // 32), dtype=torch.uint8, device=dev)

        def call():
            part = _hip.act_search_losses_mxfp4([w], x_sq, table, rule, rtable=rtable)
            _hip.quantize_mxfp4_scaled(w, table[2], rule, codes, scales)
            return part, codes, scales
        return [w, table, rtable, x_sq], call

    _, call = make()
    want = [t.cpu().clone() for t in call()]
    torch.cuda.synchronize(dev)
    with stream_gate.ordered(dev) as st:
        st.case = "mxfp4 act entries"
        tensors, call = make()
        got = [t.cpu() for t in stream_gate.run_tensors(st, tensors, call)]
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
