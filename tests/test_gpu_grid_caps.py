"""Every capped-grid kernel on its later trips (the table beside the `diag` build).

Most launches in csrc cap their grid and let each wave or thread walk its work in a grid-stride
loop; the rest of the suite runs those loops once per wave.  Here every such kernel runs them
several times, two ways:

  (a) test_caps_at_small_shapes (the cap_* cases): at small shapes under the diagnostics build's
      `max_blocks` (caps 1, 2, 3 and 7), every buffer out of a guard-band arena
      (test_gpu_bounds.Call: both fill polarities, so a skipped item is seen whatever the
      allocator held), every output byte against the independent reference of that kernel's
      existing test AND against the same call without the cap;
  (b) test_past_compiled_caps (the past_cap_* cases): the shipped library, no tuning, at the
      smallest shape past the compiled cap, outputs and workspaces pre-filled with junk.  Each
      case restates the launch arithmetic (the csrc line it mirrors is named) and asserts that its
      shape is past the cap, so a raised cap fails the case instead of letting it pass without a
      second trip.

One test id per part, the failing case named in the failure: a case takes milliseconds.

NaN payloads of the loss partials and of the fp64 loss sums are not part of their definition
(tests/test_act_search.py): against the oracle NaN positions are compared, against the uncapped
call every bit."""
import contextlib
import ctypes
import itertools

import numpy as np
import pytest
import torch

from oracle import awq_oracle as orc
from test_gpu_bounds import COMBOS, Call, _ids, quant_expect, weights
from test_gpu_fold import cpu_fold
from test_gpu_output_error import check_exact, exact_case
from test_gpu_output_error import run as run_output_error
from test_gpu_qerror import expect as expect_qerror
from test_gpu_qerror import hand_built, packed_of

pytestmark = pytest.mark.gpu

BF16, F16, F32, F64, I32 = torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int32
CAPS = (1, 2, 3, 7)          # 7: 28 waves / 1792 lanes, which leave most cases a ragged last trip


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from awq_quantizer import _hip
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    return dev


def _lib():
    """The library of the moment: the diagnostics build inside _hip.tuning(), else the shipped one."""
    from awq_quantizer import _hip
    return _hip.load_library()


def _code(dtype):
    from awq_quantizer import _hip
    return _hip.AWQ_DTYPE[dtype]


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def capped(c: Call, launch, **tune):
    """c.run(launch) without a cap, then under every cap of CAPS.  Every run starts from both fill
    polarities and compares every output byte with the case's expectations (the independent
    reference); every capped run's output bytes must also equal the uncapped run's.  tune: other
    diagnostics settings that select the kernel under test (they hold for the uncapped run too)."""
    from awq_quantizer import _hip

    def one(cap):
        kw = dict(tune, **({"max_blocks": cap} if cap else {}))
        try:
            with (_hip.tuning(**kw) if kw else contextlib.nullcontext()):
                c.run(launch)
        except AssertionError as e:
            raise AssertionError(f"max_blocks={cap}: {e}") from None
        return {b.name: b.region.u8.cpu().clone() for b in c.bufs if b.expect is not None}

    base = one(0)
    for cap in CAPS:
        for name, got in one(cap).items():
            assert torch.equal(got, base[name]), f"max_blocks={cap}: '{name}' differs from the uncapped call's bytes"


def trips(items: int, per_block: int, cap: int) -> int:
    """Trips of the busiest wave / thread when `items` are dealt to `cap` blocks of `per_block`."""
    return -(-items // (per_block * cap))


# ================================================================ (a) the diagnostics cap
# ---------------------------------------------------------------- act_loss_kernel
def loss_items(R, K, gs):
    """Kernel items of act_loss_kernel (awq_actsearch.hip group_lane<EPL>: nrb * G): 16 elements per
    lane for the ring group sizes, else 8; 64 / (gs / EPL) rows of one group column per item."""
    epl = 16 if gs in (32, 64, 128, 256) else 8
    gpw = 64 // (gs // epl)
    return -(-R // gpw) * (K // gs)


LOSS_SETS = [((37,), 512, True), ((70, 5, 33), 1024, False)]     # rows of the linears, K, NaN
_LOSS = {}


def loss_inputs(rows, K, dtype, gs, nan):
    """Weights whose LAST row block holds a constant group (and, nan, a NaN): with g = item / nrb
    the last group column's last row block is the last item, a later trip under every cap that
    loops at all.  x_sq, a 12-row table (its first n rows are a table of n candidates), 1 / table."""
    key = (rows, K, dtype, gs, nan)
    if key not in _LOSS:
        g = torch.Generator().manual_seed(K + gs + len(rows))
        ws = [(torch.randn(r, K, generator=g) * 0.02).to(dtype) for r in rows]
        last = ws[-1]
        last[-1, K - gs:] = 0.25                                   # constant group
        if nan:
            last[-1, K - 2 * gs + 3 if K >= 2 * gs else 3] = float("nan")
            if K < 2 * gs:                                          # one group per row: keep the constant group
                last[-2, :] = 0.25
        xm = torch.exp2(torch.rand(K, generator=g) * 6 - 3).float()
        xs = (torch.rand(K, generator=g) ** 4 + 1e-4).float()
        table = orc.act_scale_table(xm, None, 12)
        _LOSS[key] = (ws, xs, table, torch.ones((), dtype=F32) / table)
    return _LOSS[key]


def _loss_case(dev, ws, xs, table, rtable, opart, gs, bits, sym):
    """awq_act_search_losses of every linear into one `part`, then awq_act_search_select on it:
    part, losses, best and s_best out of the arena, `work` holding the fill."""
    n_grid, K = table.shape
    groups = [w.shape[0] * (K // gs) for w in ws]
    stride = sum(groups)
    assert opart.shape == (n_grid, stride)
    losses, best = orc.act_search_select(opart)
    c = Call(dev, seed=gs + bits + n_grid)
    wb = [c.inp(f"w{i}", w) for i, w in enumerate(ws)]
    tb, rb, xb = c.inp("table", table), c.inp("rtable", rtable), c.inp("x_sq", xs)
    pb = c.out("part", opart, nan_dtype=F32)
    kb = c.work("work", 8 * n_grid * (-(-stride // 1024)))
    lb = c.out("losses", losses, nan_dtype=F64)
    bb = c.out("best", torch.tensor([best], dtype=I32))
    sb = c.out("s_best", table[best])
    code = _code(ws[0].dtype)

    def launch():
        lib, off = _lib(), 0
        for w, b, ng in zip(ws, wb, groups):
            rc = lib.awq_act_search_losses(b.ptr, code, w.shape[0], K, gs, bits, int(sym), tb.ptr, rb.ptr, n_grid,
                                           xb.ptr, pb.at(4 * off), stride, _stream(dev))
            if rc:
                return rc
            off += ng
        return lib.awq_act_search_select(pb.ptr, n_grid, stride, tb.ptr, K, kb.ptr, lb.ptr, bb.ptr, sb.ptr,
                                         _stream(dev))
    capped(c, launch)


def cap_act_losses(dtype, gs, bits, sym):
    """The ring group sizes (gs 256: two DMAs per candidate, gs 32: partial DMAs) and the ringless
    ones; 1, 2, 3 and 12 candidates (the last reload lands in slot 1, 0, 1, 0; one candidate: the
    item's only DMA is followed by the reload alone); row counts that leave the last row block of
    every group column partly invalid.  The ring's handoff between two items of one wave runs under
    every cap whose waves get a second item: asserted."""
    dev = _dev()
    for rows, K, nan in LOSS_SETS:
        ws, xs, table, rtable = loss_inputs(rows, K, dtype, gs, nan)
        items = [loss_items(w.shape[0], K, gs) for w in ws]
        assert trips(max(items), 4, 3) >= 2                        # caps 1, 2, 3: a second item per wave
        if len(rows) > 1:
            assert trips(max(items), 4, 7) >= 2
        if gs != 512:                                               # (gs 512: one row per item, no row-block tail)
            assert all(w.shape[0] % (64 // (gs // (16 if gs in (32, 64, 128, 256) else 8))) for w in ws)
        _, _, opart = orc.act_search_losses(ws, xs, table, gs, bits, sym)    # once; candidates are independent
        assert bool(torch.isnan(opart).any()) == nan
        for n in (1, 2, 3, 12):
            try:
                _loss_case(dev, ws, xs, table[:n].contiguous(), rtable[:n].contiguous(), opart[:n].contiguous(), gs,
                           bits, sym)
            except AssertionError as e:
                raise AssertionError(f"rows {rows} K {K} n_grid {n}: {e}") from None


# ---------------------------------------------------------------- group_absmax_kernel + the column sums
def cap_weight_mean(gs, dtype):
    """awq_weight_colsum's two-pass path (group sizes outside 32 .. 256) for linears of 1, 63, 65 and
    300 rows writing their slices of one `partial`, then awq_column_mean: what _hip.weight_mean
    does, out of the arena.  gmax_work is read by the second pass: it starts from the fill.
    (Group size 128 reaches group_absmax_kernel only from a pointer off 16-B alignment, which the
    entry point refuses: weight_colsum_refuses_element_aligned_weights.)"""
    dev = _dev()
    K, rows = 1024, (1, 63, 65, 300)
    assert K % gs == 0 and gs not in (32, 64, 128, 256)
    gpw = 64 // (gs // 8)
    assert trips(-(-rows[-1] // gpw) * (K // gs), 4, 7) >= 2       # awq_actsearch.hip launch_weight_colsum: items
    ws = [weights((r, K), dtype, r + gs, nan=False, scale=0.05) for r in rows]
    nblk = [-(-r // 256) for r in rows]
    parts = []
    for w, nb in zip(ws, nblk):
        pt = torch.empty((nb, K), dtype=F64)
        assert orc.lib().oracle_weight_colsum(ctypes.c_void_p(w.data_ptr()), orc.DTYPE_CODES[dtype], w.shape[0], K, gs,
                                              ctypes.c_void_p(pt.data_ptr())) == 0
        parts.append(pt)
    c = Call(dev, seed=gs)
    wb = [c.inp(f"w{i}", w) for i, w in enumerate(ws)]
    gb = [c.work(f"gmax_work{i}", 4 * r * (K // gs)) for i, r in enumerate(rows)]
    pb = c.out("partial", torch.cat(parts))
    ob = c.out("w_mean", orc.weight_mean(ws, gs))
    c.build()
    assert all(b.addr % 16 == 0 for b in wb)

    def launch():
        lib, off = _lib(), 0
        for w, b, gw, nb in zip(ws, wb, gb, nblk):
            rc = lib.awq_weight_colsum(b.ptr, _code(dtype), w.shape[0], K, gs, gw.ptr, pb.at(8 * off * K), _stream(dev))
            if rc:
                return rc
            off += nb
        return lib.awq_column_mean(pb.ptr, sum(nblk), K, float(sum(rows)), ob.ptr, _stream(dev))
    capped(c, launch)


def weight_colsum_refuses_element_aligned_weights():
    """launch_weight_colsum sends group sizes 32 .. 256 to group_absmax_kernel when w is off 16-B
    alignment, but awq_weight_colsum returns AWQ_EINVAL for such a pointer before any launch: the
    branch cannot be reached through the C ABI, so it has no capped case."""
    dev = _dev()
    K, gs = 256, 128
    buf = torch.zeros(3 * K + 8, dtype=BF16, device=dev)
    w = buf[1:1 + 3 * K]
    assert w.data_ptr() % 16 == 2
    gmax = torch.zeros(3 * (K // gs), dtype=F32, device=dev)
    part = torch.zeros(K, dtype=F64, device=dev)
    assert _lib().awq_weight_colsum(_p(w), _code(BF16), 3, K, gs, _p(gmax), _p(part), _stream(dev)) != 0
    assert not gmax.any() and not part.any()


# ---------------------------------------------------------------- apply_scale(_any)_kernel, awq_fold_any_kernel
def cap_apply_input_scale(K, dtype):
    """K = 1000 from aligned pointers: eight elements per lane; K = 203: one element per lane."""
    dev = _dev()
    rows = 33
    vec = K % 8 == 0
    assert trips(rows * K // 8 if vec else rows * K, 256, 7) >= 2  # awq_actsearch.hip launch_apply_scale
    w = weights((rows, K), dtype, K, nan=False)
    s = torch.exp2(torch.rand(K, generator=torch.Generator().manual_seed(3)) * 4 - 2).float()
    c = Call(dev, seed=K)
    wb, sb = c.inp("w", w), c.inp("s", s)
    ob = c.out("out", orc.apply_input_scale(w, s))
    c.build()
    assert wb.addr % 16 == 0 and sb.addr % 16 == 0 and ob.addr % 16 == 0
    capped(c, lambda: _lib().awq_apply_input_scale(wb.ptr, _code(dtype), rows, K, sb.ptr, ob.ptr, _stream(dev)))


def cap_fold_rows(shape, dtype):
    """The one-element-per-lane kernel: K % 8 != 0, and K = 1 (the row lookup's i / K shortcut)."""
    dev = _dev()
    rows, K = shape
    assert K % 8 != 0 and trips(rows * K, 256, 7) >= 2             # awq_fold.hip launch_fold_rows
    w = weights(shape, dtype, rows + K, nan=False)
    s = torch.exp2(torch.rand(rows, generator=torch.Generator().manual_seed(rows)) * 4 - 2).float()
    c = Call(dev, seed=rows + K)
    wb, sb = c.inp("w", w), c.inp("row_scale", s)
    ob = c.out("out", cpu_fold(w, s))
    capped(c, lambda: _lib().awq_fold_rows(wb.ptr, _code(dtype), rows, K, sb.ptr, ob.ptr, _stream(dev)))


# ---------------------------------------------------------------- qerror_group_kernel
def cap_quant_error(gs, dtype, bits, sym):
    """(33, 1000): a tail group of 8 (gs 16), 16 (gs 24) and none (gs 100); a constant group and a NaN
    group; totals asked for, so the level-2 reduction reads what the later trips wrote."""
    dev = _dev()
    rows, K = 33, 1000
    G = -(-K // gs)
    assert trips(rows * G, 4, 7) >= 2                              # awq_qerror.hip awq_quant_error: (ng + 3) / 4
    qmin = orc.qrange(bits, sym)[0]
    w = weights((rows, K), dtype, rows + K + bits, const=gs)
    ref = orc.quantize(w, bits=bits, group_size=gs, symmetric=sym)
    e = expect_qerror(w, ref)
    stats = np.stack([e[k].reshape(-1) for k in ("group_abs", "group_sq", "group_w_sq", "group_max")])
    nbytes = _lib().awq_quant_error_work_bytes(rows, K, gs)
    assert nbytes > 0 and e["totals"][4] > 0
    c = Call(dev, seed=K + bits + gs)
    wb = c.inp("w", w)
    qb = c.inp("qweight", orc.pack_rows(ref["tensor_q"].reshape(rows, K), bits, qmin))
    zb = c.inp("qzeros", orc.pack_rows(ref["zero_points"], bits, qmin))
    sb = c.inp("scales", ref["scales"])
    gb = c.out("group_stats", stats)
    nb = c.out("group_nonfinite", e["group_nonfinite"].reshape(-1).astype(np.int32))
    kb = c.work("work", nbytes)
    tb = c.out("totals", e["totals"])
    capped(c, lambda: _lib().awq_quant_error(wb.ptr, _code(dtype), rows, K, gs, bits, int(sym), qb.ptr, zb.ptr, sb.ptr,
                                             gb.ptr, nb.ptr, kb.ptr, tb.ptr, _stream(dev)))


# ---------------------------------------------------------------- awq_generic_kernel
GENERIC_TUNE = {"no_rowgroup": 1, "gen_noreg": 1}    # bf16 gs 100 off the row-segment kernel, fp64 off the LDS span


def cap_generic(what, gs, dtype, bits, sym):
    """awq_generic_kernel<D, false> (plain quantize and the exact group parameters) and <D, true>
    (clip search, n_candidates 3; the search takes group sizes up to 512) at (33, 1000): group size
    100 gives ten groups per row, so a full span and a short last span per row (spans of 8 groups
    at 4 bits, 4 at 8 bits); group size 1000 one group and one span per row."""
    dev = _dev()
    rows, K = 33, 1000
    G, per = -(-K // gs), 32 // bits
    assert trips(rows * -(-G // per), 4, 7) >= 2                   # awq_generic.hip launch_generic: rows * ceil(G / per)
    w = weights((rows, K), dtype, rows + gs + bits, nan=(what != "params"), const=gs)
    c = Call(dev, seed=gs + bits)
    wb = c.inp("w", w)
    if what == "params":
        s, z = orc.group_params(w, rows, K, gs, bits, sym)
        ob = [c.out("scales", s), c.out("zeros", z)]
    else:
        want = quant_expect(w, rows, K, gs, bits, sym, (4, 3) if what == "search" else None)
        ob = [c.out(n, want[n]) for n in ("qweight", "qzeros", "scales", "tensor_q", "zeros")]
    head = lambda: (wb.ptr, _code(dtype), rows, K, gs, bits, int(sym), 0)
    tail = lambda: (*[b.ptr for b in ob], _stream(dev))
    if what == "params":
        launch = lambda: _lib().awq_group_params_ex(*head(), *tail())
    elif what == "search":
        launch = lambda: _lib().awq_quantize_search_ex(*head(), 4, 3, *tail())
    else:
        launch = lambda: _lib().awq_quantize_groups_ex(*head(), *tail())
    capped(c, launch, **GENERIC_TUNE)


# ---------------------------------------------------------------- awq_apply_kernel, awq_pack_kernel, awq_dequant_kernel
def cap_apply_params_ex():
    """quantize()'s int32 tensor_q dequantized with fp16 parameters (mode 1, both ops fp16) at
    (33, 1000), group size 100."""
    dev = _dev()
    from awq_quantizer import _hip
    rows, K, gs = 33, 1000, 100
    G = K // gs
    assert trips(rows * K, 256, 7) >= 2                            # awq_generic.hip launch_apply
    g = torch.Generator().manual_seed(gs)
    x = torch.randint(-8, 8, (rows, K), generator=g, dtype=I32)
    s16 = (torch.rand(rows, G, generator=g) * 0.01 + 1e-3).to(F16)
    z16 = torch.randint(-8, 8, (rows, G), generator=g).to(F16)
    col = torch.arange(K) // gs
    want = orc.apply_promoted(x, s16[:, col].contiguous(), z16[:, col].contiguous(), -8, 7, 1, False)
    c = Call(dev, seed=gs)
    xb, sb, zb = c.inp("x", x), c.inp("scales", s16.double()), c.inp("zeros", z16.double())
    ob = c.out("out", want)
    capped(c, lambda: _lib().awq_apply_params_ex(xb.ptr, _hip.APPLY_DTYPE[I32], rows, K, gs, sb.ptr, zb.ptr, -8, 7, 1,
                                                 _hip.APPLY_OP_DTYPE[F16], _hip.APPLY_OP_DTYPE[F16], 0, ob.ptr,
                                                 _stream(dev)))


def cap_pack_rows(bits, qmin):
    dev = _dev()
    rows, n = 33, 1000
    assert trips(rows * -(-n // (32 // bits)), 256, 7) >= 2        # awq_generic.hip launch_pack
    g = torch.Generator().manual_seed(n + bits)
    v = torch.randint(qmin, qmin + (1 << bits), (rows, n), generator=g, dtype=I32)
    v[0, 0] = -2 ** 31
    c = Call(dev, seed=n + bits)
    vb = c.inp("v", v)
    ob = c.out("packed", orc.pack_rows(v, bits, qmin))
    capped(c, lambda: _lib().awq_pack_rows(vb.ptr, rows, n, bits, qmin, ob.ptr, _stream(dev)))


def cap_dequantize(bits, sym, dtype):
    """The int32 tensor_q path (awq_dequantize -> awq_dequant_kernel) at (33, 1000), group size 100,
    with a NaN group."""
    dev = _dev()
    rows, K, gs = 33, 1000, 100
    assert trips(rows * K, 256, 7) >= 2                            # awq_generic.hip launch_dequant
    w = weights((rows, K), dtype, rows + K + bits, const=gs)
    tq, sc, zp = orc.quantize_groups(w, rows, K, gs, bits, sym)
    tq = tq.reshape(rows, K)
    want = orc.dequantize({"tensor_q": tq, "scales": sc, "zero_points": zp, "group_size": torch.tensor(gs)})
    assert bool(torch.isnan(want).any())
    c = Call(dev, seed=K + bits)
    qb, zb, sb = c.inp("tensor_q", tq), c.inp("zeros", zp), c.inp("scales", sc)
    ob = c.out("out", want)
    capped(c, lambda: _lib().awq_dequantize(qb.ptr, sb.ptr, zb.ptr, rows, K, gs, ob.ptr, _stream(dev)))


# ---------------------------------------------------------------- outerr_mfma_kernel, outerr_generic_kernel
def cap_output_error(dtype, shape, gs, row_tile):
    """max_blocks makes the tile loop of both kernels reachable (2 x 2 and 2 x 1 tiles).  Exact
    data (test_gpu_output_error.exact_case): err equals the float64 product exactly and err_sq /
    ref_sq are within that file's (T + 2) 2^-24, checked on the uncapped call's outputs; every capped
    call must then reproduce those bytes from both fills."""
    dev = _dev()
    from awq_quantizer import _hip
    N, K, T = shape
    tiles = -(-N // row_tile) * (-(-T // 128))                     # awq_outerr.hip awq_output_error: tiles
    assert tiles >= 2 and (dtype == BF16) == (gs in (32, 64, 128, 256))
    case = exact_case(N, K, T, gs, 4, False, dtype, True, seed=N + K + T)
    want = run_output_error(dev, case)
    check_exact(case, want, T)
    assert np.array_equal(want[2].astype(np.float64), case["E"])
    c = Call(dev, seed=N + gs)
    wb, qb, zb = c.inp("w", case["w"]), c.inp("qweight", case["qweight"]), c.inp("qzeros", case["qzeros"])
    sb, cb, xb = c.inp("scales", case["scales"].view(np.int16)), c.inp("col_scale", case["col"]), c.inp("x", case["x"])
    kb = c.work("work", _lib().awq_output_error_work_bytes(N, T))
    eb, rb, fb = c.out("err_sq", want[0]), c.out("ref_sq", want[1]), c.out("err", want[2])
    capped(c, lambda: _lib().awq_output_error(wb.ptr, _hip.AWQ_DTYPE[dtype], N, K, gs, 4, 0, qb.ptr, zb.ptr, sb.ptr,
                                              cb.ptr, xb.ptr, T, K, kb.ptr, eb.ptr, rb.ptr, fb.ptr, _stream(dev)))


# ================================================================ (b) the shipped library past its caps
def _randn(shape, dtype, dev, seed, scale=0.02, block=2048):
    """randn * scale on the device, generated in row slices (no fp32 temporary of the whole tensor)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.empty(shape, dtype=dtype, device=dev)
    for r0 in range(0, shape[0], block):
        n = min(block, shape[0] - r0)
        x[r0:r0 + n] = (torch.randn(n, *shape[1:], device=dev, generator=g) * scale).to(dtype)
    return x


def _junk(shape, dtype, dev, byte):
    """A device tensor whose every byte is `byte` (call sites use different bytes: equal results
    mean that both calls wrote them)."""
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(-1).view(torch.uint8).fill_(byte)
    return t


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8).cpu(),
                                                                     b.contiguous().view(-1).view(torch.uint8).cpu())


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _ok(rc):
    from awq_quantizer import _hip
    assert rc == 0, _hip.last_error()


def assert_past_cap(work, per_block, cap, what):
    """blocks_for / grid_for of csrc: the grid is min(ceil(work / per_block), cap) blocks; the case
    needs more work than the capped grid takes in one trip."""
    assert -(-work // per_block) > cap, f"{what}: {work} work units no longer pass the cap of {cap} blocks x {per_block}"


LOSS_CAP = 256 * 32           # awq_actsearch.hip launch_act_losses: blocks_for(.., 4, 256 * 32)
ABSMAX_CAP = 256 * 64         # awq_actsearch.hip launch_weight_colsum: blocks_for(items, 4, 256 * 64)
SCALE_CAP = 256 * 64          # awq_actsearch.hip launch_apply_scale: blocks_for(.., 256, 256 * 64)
FOLD_CAP = 65536              # awq_fold.hip launch_fold_rows: if (blocks > 65536) blocks = 65536
QERROR_CAP = 256 * 64         # awq_qerror.hip awq_quant_error: std::min((ng + 3) / 4, 256 * 64)
GENERIC_CAP = 256 * 16        # awq_generic.hip launch_generic / launch_apply / launch_pack: grid_for(.., 256 * 16)
SLICE = 512                   # columns the oracle is run on for the loss cases: the last group columns


def _losses(dev, w, xs, table, rtable, gs, fill, blocks=None):
    """awq_act_search_losses into a junk-filled part; blocks: the rows as a list of row blocks."""
    R, K = w.shape
    n_grid, G = table.shape[0], K // gs
    part = _junk((n_grid, R * G), F32, dev, fill)
    off = 0
    for r0, r1 in (blocks or [(0, R)]):
        _ok(_lib().awq_act_search_losses(_p(w[r0:r1]), _code(w.dtype), r1 - r0, K, gs, 4, 0, _p(table), _p(rtable),
                                         n_grid, _p(xs), ctypes.c_void_p(part.data_ptr() + 4 * off), R * G,
                                         _stream(dev)))
        off += (r1 - r0) * G
    torch.cuda.synchronize(dev)
    return part


def past_cap_act_losses(dtype, gs, shape, grids):
    """act_loss_kernel's second item per wave in the shipped library: the ring handoff (gs 128; the
    last row block holds one valid row) and the ringless loop (gs 512).  The later trips are the
    last group columns (group_lane: g = item / nrb), so the oracle runs on the last 512 columns —
    include/awq_hip.h: part[i * part_stride + r * G + g] per linear — and the whole tensor must
    equal its row blocks given as a list, each block below the cap."""
    dev = _dev()
    from awq_quantizer import _hip
    R, K = shape
    G = K // gs
    ring = gs in (32, 64, 128, 256)
    host_items = -(-R // (64 // (gs // 8))) * G                    # launch_act_losses: items
    assert_past_cap((host_items + 1) // 2 if ring else host_items, 4, LOSS_CAP, "act_loss_kernel")
    assert loss_items(R, K, gs) > 4 * LOSS_CAP                     # the kernel's own item count (group_lane<EPL>)
    blocks = [(0, 4096), (4096, R)] if R > 4097 else [(0, 2048), (2048, R)]
    for r0, r1 in blocks:
        assert loss_items(r1 - r0, K, gs) <= 4 * LOSS_CAP
    w = _randn(shape, dtype, dev, seed=gs)
    w[R - 1, K - gs:] = 0.25                                        # a constant group in the last item
    g = torch.Generator().manual_seed(gs)
    xm = torch.exp2(torch.rand(K, generator=g) * 6 - 3).float()
    xs = (torch.rand(K, generator=g) ** 4 + 1e-4).float()
    wc = w[:, K - SLICE:].cpu().contiguous()
    for n_grid in grids:
        table = orc.act_scale_table(xm, None, n_grid)
        td, xd = table.to(dev), xs.to(dev)
        rd = _hip.act_recip_table(td)
        whole = _losses(dev, w, xd, td, rd, gs, 0xA5)
        _, _, opart = orc.act_search_losses([wc], xs[K - SLICE:].contiguous(), table[:, K - SLICE:].contiguous(), gs, 4,
                                            False)
        got = whole.view(n_grid, R, G)[:, :, G - SLICE // gs:].contiguous().cpu()
        assert torch.equal(got.reshape(n_grid, -1).view(I32), opart.view(I32)), f"n_grid {n_grid}: last columns"
        assert _same(whole, _losses(dev, w, xd, td, rd, gs, 0x3C, blocks)), f"n_grid {n_grid}: row blocks"


def past_cap_weight_mean():
    """group_absmax_kernel past 65536 items: (8193, 4096) at group size 512.  The last group column
    against the oracle (w_mean is column-wise given the groups), `partial` against the row blocks."""
    dev = _dev()
    R, K, gs = 8193, 4096, 512
    assert_past_cap(-(-R // (64 // (gs // 8))) * (K // gs), 4, ABSMAX_CAP, "group_absmax_kernel")
    w = _randn((R, K), BF16, dev, seed=5, scale=0.05)

    def colsum(r0, r1, fill):
        gmax = _junk(((r1 - r0) * (K // gs),), F32, dev, fill)
        part = _junk((-(-(r1 - r0) // 256), K), F64, dev, fill)
        _ok(_lib().awq_weight_colsum(_p(w[r0:r1]), _code(BF16), r1 - r0, K, gs, _p(gmax), _p(part), _stream(dev)))
        return part

    whole = colsum(0, R, 0xA5)
    out = _junk((K,), F32, dev, 0xA5)
    _ok(_lib().awq_column_mean(_p(whole), whole.shape[0], K, float(R), _p(out), _stream(dev)))
    want = orc.weight_mean([w[:, K - gs:].cpu().contiguous()], gs)
    assert torch.equal(out[K - gs:].cpu().view(I32), want.view(I32))
    blocks = torch.cat([colsum(0, 4096, 0x3C), colsum(4096, R, 0x3C)])
    assert _same(whole, blocks)


def past_cap_apply_input_scale(shape):
    """(8193, 4096): eight elements per lane past 16384 blocks; (1025, 4100): one element per lane."""
    dev = _dev()
    R, K = shape
    vec = K % 8 == 0
    assert_past_cap(R * K // 8 if vec else R * K, 256, SCALE_CAP, "apply_scale kernels")
    w = _randn(shape, BF16, dev, seed=K)
    s = torch.exp2(torch.rand(K, generator=torch.Generator().manual_seed(3)) * 4 - 2).float()
    sd = s.to(dev)
    out = _junk(shape, BF16, dev, 0xA5)
    assert (w.data_ptr() | sd.data_ptr() | out.data_ptr()) % 16 == 0
    _ok(_lib().awq_apply_input_scale(_p(w), _code(BF16), R, K, _p(sd), _p(out), _stream(dev)))
    assert _same(out.cpu(), orc.apply_input_scale(w.cpu(), s))


def past_cap_fold_rows():
    dev = _dev()
    R, K = 4097, 4100
    assert K % 8 != 0
    assert_past_cap(R * K, 256, FOLD_CAP, "awq_fold_any_kernel")
    w = _randn((R, K), BF16, dev, seed=7, scale=1.0)
    s = torch.exp2(torch.rand(R, generator=torch.Generator().manual_seed(R)) * 4 - 2).float()
    out = _junk((R, K), BF16, dev, 0xA5)
    sd = s.to(dev)
    _ok(_lib().awq_fold_rows(_p(w), _code(BF16), R, K, _p(sd), _p(out), _stream(dev)))
    assert _same(out.cpu(), cpu_fold(w, s))


def past_cap_quant_error():
    """qerror_group_kernel past 65536 groups: (1025, 1024) at group size 16, a hand-built packed
    result.  The later trips are the last row's groups: the last two rows against the numpy
    restatement, the totals against the oracle's level-2 sums of the GPU's own group planes, the
    whole against its row blocks."""
    dev = _dev()
    R, K, gs, bits = 1025, 1024, 16, 4
    G = K // gs
    assert_past_cap(R * G, 4, QERROR_CAP, "qerror_group_kernel")
    w = _randn((R, K), BF16, dev, seed=9, scale=0.05)
    ref = hand_built((R, K), gs, bits, False, seed=3, special=False)
    pk = {k: v.to(dev) for k, v in packed_of(ref, (R, K)).items()}

    def run(r0, r1, fill, totals):
        n = r1 - r0
        stats, bad = _junk((4, n * G), F32, dev, fill), _junk((n * G,), I32, dev, fill)
        nbytes = _lib().awq_quant_error_work_bytes(n, K, gs)
        work = _junk((nbytes // 8,), F64, dev, fill) if totals else None
        tot = _junk((5,), F64, dev, fill) if totals else None
        _ok(_lib().awq_quant_error(_p(w[r0:r1]), _code(BF16), n, K, gs, bits, 0, _p(pk["qweight"][r0:r1]),
                                   _p(pk["qzeros"][r0:r1]), _p(pk["scales"][r0:r1]), _p(stats), _p(bad),
                                   _p(work) if totals else None, _p(tot) if totals else None, _stream(dev)))
        return stats, bad, tot

    stats, bad, tot = run(0, R, 0xA5, True)
    tail = {k: (v[R - 2:] if v.dim() == 2 else v) for k, v in ref.items()}
    e = expect_qerror(w[R - 2:].cpu(), tail)
    got = stats.view(4, R, G)[:, R - 2:].contiguous().cpu().numpy()
    for i, k in enumerate(("group_abs", "group_sq", "group_w_sq", "group_max")):
        assert np.array_equal(got[i].view(np.int32), e[k].view(np.int32)), k
    assert np.array_equal(bad.view(R, G)[R - 2:].cpu().numpy(), e["group_nonfinite"])
    sums, _ = orc.act_search_select(stats[:3].cpu())
    want = np.array([*sums.tolist(), float(stats[3].max()), float(bad.sum())], dtype=np.float64)
    assert np.array_equal(tot.cpu().numpy().view(np.int64), want.view(np.int64))
    s0, b0, _ = run(0, 1024, 0x3C, False)
    s1, b1, _ = run(1024, R, 0x3C, False)
    assert _same(stats.view(4, R, G), torch.cat([s0.view(4, 1024, G), s1.view(4, 1, G)], dim=1))
    assert _same(bad, torch.cat([b0, b1]))


def past_cap_generic_group_params():
    """awq_generic_kernel<bf16, false> past 16384 spans: the exact parameters of (4097, 4096), gs 128."""
    dev = _dev()
    R, K, gs, bits = 4097, 4096, 128, 4
    assert_past_cap(R * -(-(K // gs) // (32 // bits)), 4, GENERIC_CAP, "awq_generic_kernel (group_params)")
    w = _randn((R, K), BF16, dev, seed=11)
    s, z = _junk((R, K // gs), F64, dev, 0xA5), _junk((R, K // gs), F64, dev, 0xA5)
    _ok(_lib().awq_group_params_ex(_p(w), _code(BF16), R, K, gs, bits, 0, 0, _p(s), _p(z), _stream(dev)))
    ws, wz = orc.group_params(w.cpu(), R, K, gs, bits, False)
    assert _same(s.cpu(), ws.reshape(R, -1)) and _same(z.cpu(), wz.reshape(R, -1))


def past_cap_generic_quantize():
    """awq_generic_kernel past 16384 spans: (16385, 520) at group size 520 (> 512: no other kernel)."""
    dev = _dev()
    R, K, gs, bits = 16385, 520, 520, 4
    assert_past_cap(R * 1, 4, GENERIC_CAP, "awq_generic_kernel (quantize)")
    w = _randn((R, K), BF16, dev, seed=13)
    w[R - 1, 5] = float("nan")
    per = 32 // bits
    qw, qz = _junk((R, K // per), I32, dev, 0xA5), _junk((R, 1), I32, dev, 0xA5)
    sc = _junk((R, 1), F16, dev, 0xA5)
    _ok(_lib().awq_quantize_groups_ex(_p(w), _code(BF16), R, K, gs, bits, 0, 0, _p(qw), _p(qz), _p(sc), None, None,
                                      _stream(dev)))
    want = quant_expect(w.cpu(), R, K, gs, bits, False)
    assert _same(qw.cpu(), want["qweight"].reshape(R, -1)) and _same(qz.cpu(), want["qzeros"].reshape(R, -1))
    assert _same(sc.cpu(), want["scales"].reshape(R, -1))


def past_cap_apply_params_and_pack_rows():
    """awq_apply_kernel and awq_pack_kernel past 4096 blocks x 256 work units ((1025, 1024) elements,
    (1025, 8192) -> 1025 x 1024 words).  awq_dequant_kernel needs no case: test_gpu_parity's
    test_golden_hashed dequantizes 1024 x 4096 int32 values against the golden hashes."""
    dev = _dev()
    from awq_quantizer import _hip
    R, K, gs = 1025, 1024, 128
    assert_past_cap(R * K, 256, GENERIC_CAP, "awq_apply_kernel")
    g = torch.Generator().manual_seed(17)
    x = torch.randint(-8, 8, (R, K), generator=g, dtype=I32)
    s16 = (torch.rand(R, K // gs, generator=g) * 0.01 + 1e-3).to(F16)
    z16 = torch.randint(-8, 8, (R, K // gs), generator=g).to(F16)
    col = torch.arange(K) // gs
    want = orc.apply_promoted(x, s16[:, col].contiguous(), z16[:, col].contiguous(), -8, 7, 1, False)
    out = _junk((R, K), F16, dev, 0xA5)
    xd, sd, zd = x.to(dev), s16.double().to(dev), z16.double().to(dev)
    _ok(_lib().awq_apply_params_ex(_p(xd), _hip.APPLY_DTYPE[I32], R, K, gs, _p(sd), _p(zd), -8, 7, 1,
                                   _hip.APPLY_OP_DTYPE[F16], _hip.APPLY_OP_DTYPE[F16], 0, _p(out), _stream(dev)))
    assert _same(out.cpu(), want)
    n = 8192
    assert_past_cap(R * (n // 8), 256, GENERIC_CAP, "awq_pack_kernel")
    v = torch.randint(0, 16, (R, n), generator=g, dtype=I32)
    packed = _junk((R, n // 8), I32, dev, 0xA5)
    vd = v.to(dev)
    _ok(_lib().awq_pack_rows(_p(vd), R, n, 4, 0, _p(packed), _stream(dev)))
    assert _same(packed.cpu(), orc.pack_rows(v, 4, 0))


# ================================================================ the two tests
def each(cases):
    """fn(*args) for every case of one test, the case named in the failure it raises (one test id
    per part rather than one per case: a case takes milliseconds, and the suite's list of ids
    stays short)."""
    for fn, args in cases:
        try:
            fn(*args)
        except AssertionError as e:
            raise AssertionError(f"{fn.__name__}{_ids(args)}: {e}") from e


def _product(fn, *axes):
    return [(fn, args) for args in itertools.product(*axes)]


def _flat(fn, outer, inner):
    return [(fn, (*o, *i)) for o in outer for i in inner]


QUANT = [(4, False), (4, True), (8, False)]
CAP_CASES = (
    _flat(cap_act_losses, itertools.product([BF16, F16, F32], [32, 128, 256, 8, 512]), QUANT)
    + [(cap_weight_mean, c) for c in [(8, BF16), (16, F16), (512, F32), (512, BF16)]]
    + [(weight_colsum_refuses_element_aligned_weights, ())]
    + _product(cap_apply_input_scale, [1000, 203], [BF16, F16, F32])
    + _product(cap_fold_rows, [(33, 203), (2000, 1)], [BF16, F16, F32])
    + _flat(cap_quant_error, [(16,), (24,), (100,)], COMBOS[:3])
    + _flat(cap_generic, [(what, gs, dtype) for what, gs in [("quantize", 100), ("quantize", 1000), ("search", 100),
                                                              ("params", 100), ("params", 1000)]
                          for dtype in (BF16, F64)], [(4, False), (8, True)])
    + [(cap_apply_params_ex, ())]
    + [(cap_pack_rows, c) for c in [(4, 0), (8, -128)]]
    + [(cap_dequantize, c) for c in [(4, False, BF16), (8, True, F16)]]
    + [(cap_output_error, c) for c in [(BF16, (130, 512, 129), 64, 128), (F16, (72, 256, 70), 16, 64)]])
PAST_CAP_CASES = (
    [(past_cap_act_losses, c) for c in [(BF16, 128, (8193, 4096), (2, 3)), (F16, 512, (4097, 4096), (3,))]]
    + [(past_cap_weight_mean, ())]
    + [(past_cap_apply_input_scale, (s,)) for s in [(8193, 4096), (1025, 4100)]]
    + [(past_cap_fold_rows, ()), (past_cap_quant_error, ()), (past_cap_generic_group_params, ()),
       (past_cap_generic_quantize, ()), (past_cap_apply_params_and_pack_rows, ())])


def test_caps_at_small_shapes():
    """(a): every capped launch under max_blocks 1, 2, 3 and 7 (the cap_* cases above)."""
    each(CAP_CASES)


def test_past_compiled_caps():
    """(b): the shipped library at the smallest shape past each compiled cap (the past_cap_* cases)."""
    each(PAST_CAP_CASES)
