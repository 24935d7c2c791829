"""Only your bytes, all of your bytes, whatever was there before: every kernel entry point of
include/awq_hip.h run out of a guard-band arena (tests/guard_arena.py).

Every case places its inputs, outputs and workspaces in one arena, outputs and workspaces sized
exactly as the header documents, and calls the C ABI twice: once on the arena's pseudo-random fill
and once on its bitwise complement.  Both runs must
  1. leave every byte outside the outputs alone (guards, gaps, the inputs, documented slack);
  2. produce the CPU expectation in every output byte — pad fields of the last qweight / qzeros
     word and NaN scale bits included — so a skipped byte (it holds the fill, wrong in at least one
     polarity) or an over-read reaching a min, max or sum (it sees other data in the two runs) fails;
  3. do so with the workspaces left holding the fill.
Expectations come from the CPU oracle, from the expectation helpers of test_gpu_qerror.py and
test_gpu_act_clip.py, and from torch's CPU ops; each is computed once per case and shared by the
two polarities.  Every case asserts the predicate that selects its kernel before it runs.
Inside stream_gate.ordered() (tests/test_stream_order_gpu.py) Call.run makes the same checks on a
non-blocking stream whose memory is stale until a device-side gate has passed; outside it nothing
changes."""
import ctypes

import numpy as np
import pytest
import torch

import stream_gate
from guard_arena import Arena
from oracle import awq_oracle as orc
from test_gpu_act_clip import expect_clip
from test_gpu_qerror import expect as expect_qerror

pytestmark = pytest.mark.gpu

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
I32 = torch.int32
ESIZE = {BF16: 2, F16: 2, F32: 4, F64: 8}
COMBOS = [(BF16, 4, False), (F16, 8, True), (F32, 4, True), (BF16, 8, False)]
_ids = lambda v: str(v).replace("torch.", "")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from awq_quantizer import _hip
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    return dev


def _lib():
    from awq_quantizer import _hip
    return _hip.load_library()


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---------------------------------------------------------------- the mechanism
class Buf:
    def __init__(self, name, nbytes, data, expect, skew, align, untouched, nan_dtype, written, pointers=False):
        self.name, self.nbytes, self.data, self.skew, self.align = name, nbytes, data, skew, align
        self.untouched, self.nan_dtype, self.written, self.pointers = untouched, nan_dtype, written, pointers
        self.expect = None if expect is None else _bytes(expect)
        self.region = None

    @property
    def ptr(self):
        return ctypes.c_void_p(self.region.data_ptr())

    @property
    def addr(self) -> int:
        return self.region.data_ptr()

    def at(self, byte_offset: int):
        assert 0 <= byte_offset <= self.nbytes
        return ctypes.c_void_p(self.region.data_ptr() + byte_offset)


def _bytes(t) -> torch.Tensor:
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).clone()


class Call:
    """One case: buffers in placement order, then run(launch) does the two polarities."""

    def __init__(self, dev, seed=1):
        self.dev, self.seed, self.bufs, self.arena = dev, seed, [], None

    def _add(self, b):
        assert self.arena is None, "buffers are declared before build()"
        self.bufs.append(b)
        return b

    def inp(self, name, t=None, *, nbytes=None, skew=0, align=256, untouched=True, expect=None, nan_dtype=None,
            pointers=False):
        """An input (contents stored after every fill).  expect: the input is also an output.
        pointers: the kernel turns these bytes into addresses or indices (descriptors, a block
        table) — in ordered mode (tests/stream_gate.py) they are never stale."""
        data = None if t is None else _bytes(t)
        return self._add(Buf(name, data.numel() if nbytes is None else nbytes, data, expect, skew, align, untouched,
                             nan_dtype, None, pointers))

    def out(self, name, expect, *, skew=0, align=256, nan_dtype=None, written=None):
        """An output of exactly the expectation's size, left holding the fill.  nan_dtype: NaN
        elements of that dtype are compared as NaN (where the definition pins no payload).
        written: bool per byte — the bytes the kernel owns; the others must keep the fill."""
        e = _bytes(expect)
        return self._add(Buf(name, e.numel(), None, e, skew, align, False, nan_dtype, written))

    def work(self, name, nbytes, *, skew=0, align=256):
        """A workspace of exactly nbytes, left holding the fill; its final contents are free."""
        return self._add(Buf(name, int(nbytes), None, None, skew, align, False, None, None))

    def build(self):
        if self.arena is None:
            self.arena = Arena(Arena.required([b.nbytes for b in self.bufs]), self.dev)
            for b in self.bufs:
                b.region = self.arena.place(b.nbytes, align=b.align, skew=b.skew, name=b.name, untouched=b.untouched)
                assert b.region.data_ptr() % b.align == b.skew and b.region.nbytes == b.nbytes
        return self

    def run(self, launch):
        self.build()
        for complement in (False, True):
            self.arena.fill(self.seed, complement)
            for b in self.bufs:
                if b.data is not None:
                    b.region.store(b.data)
            gate = stream_gate.active()
            rc = launch() if gate is None else self._ordered(gate, launch)
            if rc != 0:
                from awq_quantizer import _hip
                raise AssertionError(f"entry point returned {rc}: {_hip.last_error()}")
            torch.cuda.synchronize(self.dev)
            pol = "complement fill" if complement else "plain fill"
            try:
                self.arena.check()                                   # 1. nothing outside is written
            except AssertionError as e:
                raise AssertionError(f"[{pol}] {e}") from None
            for b in self.bufs:                                      # 2./3. every output byte, from any contents
                if b.expect is not None:
                    self._compare(b, pol)

    def _ordered(self, gate, launch):
        """Inside stream_gate.ordered(): the arena goes stale (the complement of what the call must
        find, pointer-bearing inputs excepted), and the gate, the restore and the call follow on
        the gate's stream, with stream 0 synchronised while the gate still spins."""
        buf = self.arena.buf
        shadow = buf.clone()
        rc = launch()                # not the test: the runtime loads a kernel's code at its first launch
        if rc != 0:                  # (tens of milliseconds), which must not happen behind the gate
            return rc
        torch.bitwise_not(shadow, out=buf)
        for b in self.bufs:
            if b.pointers:
                b.region.u8.copy_(shadow[b.region.start:b.region.end])
        torch.cuda.synchronize(self.dev)
        return gate.behind_gate(lambda: buf.copy_(shadow), launch)

    def _compare(self, b, pol):
        got = b.region.u8.cpu()
        ok = got == b.expect
        if b.nan_dtype is not None:
            size = ESIZE[b.nan_dtype]
            both = torch.isnan(got.view(b.nan_dtype)) & torch.isnan(b.expect.view(b.nan_dtype))
            ok = ok | both.reshape(-1, 1).expand(-1, size).reshape(-1)
        fill = self.arena.fill_of(b.region)
        if b.written is not None:
            ok = torch.where(b.written, ok, got == fill)
        if bool(ok.all()):
            return
        bad = torch.nonzero(~ok).reshape(-1)
        stale = int((got[bad] == fill[bad]).sum())
        raise AssertionError(f"[{pol}] '{b.name}': {bad.numel()} of {b.nbytes} bytes differ from the expectation, "
                             f"offsets {int(bad[0])} .. {int(bad[-1])}; {stale} of them still hold the fill")


def elem_mask(mask: torch.Tensor, size: int) -> torch.Tensor:
    """bool per element -> bool per byte"""
    return mask.reshape(-1, 1).expand(-1, size).reshape(-1).contiguous()


# ---------------------------------------------------------------- inputs
def weights(shape, dtype, seed, nan=True, scale=0.03, const=8):
    """randn x 0.03 whose first `const` elements are constant (const = group size: a constant
    group) and (nan=True) with a NaN in the tensor's last group."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(*shape, generator=g) * scale).to(dtype)
    flat = w.reshape(-1)
    flat[:min(const, flat.numel() // 2)] = 0.25
    if nan and flat.numel() > 64:
        flat[-3] = float("nan")
    return w


def rows_k(shape):
    return (1, shape[0]) if len(shape) == 1 else (shape[0], shape[1])


def quant_expect(w, rows, K, gs, bits, sym, search=None, small=False):
    """The oracle's five outputs: tensor_q / scales / zeros and the packing of the first and last."""
    qmin = orc.qrange(bits, sym)[0]
    tq, sc, zp = orc.quantize_groups(w.reshape(-1), rows, K, gs, bits, sym, search=search, small=small)
    return {"qweight": orc.pack_rows(tq.reshape(rows, K), bits, qmin), "qzeros": orc.pack_rows(zp, bits, qmin),
            "scales": sc, "tensor_q": tq, "zeros": zp}


# the streaming kernel's three qzeros layouts (csrc/awq_internal.h fast_geom)
def byte_tiles(K, gs, bits):
    return K % gs == 0 and (bits == 8 or (K // gs) % 2 == 0)


def word_tiles(K, gs, bits):
    return K % gs == 0 and bits == 4 and (K // gs) % 2 == 1


def padded_rows(K, gs, bits):
    return K % gs != 0 and K % 8 == 0


def _quant_case(dev, w, shape, gs, bits, sym, *, skew=0, search=None, small=False, outs="all"):
    """awq_quantize_groups_ex / awq_quantize_search_ex out of the arena."""
    from awq_quantizer import _hip
    lib = _lib()
    rows, K = rows_k(shape)
    want = quant_expect(w, rows, K, gs, bits, sym, search, small)
    c = Call(dev, seed=rows * K + gs + bits)
    wb = c.inp("w", w, skew=skew)
    names = ("qweight", "qzeros", "scales", "tensor_q", "zeros") if outs == "all" else ("qweight", "qzeros", "scales")
    ob = {n: c.out(n, want[n]) for n in names}
    p = lambda n: ob[n].ptr if n in ob else None
    code = _hip.AWQ_DTYPE[w.dtype]
    flags = _hip.Q_SMALL_TENSOR if small else 0

    def launch():
        if search is not None:
            return lib.awq_quantize_search_ex(wb.ptr, code, rows, K, gs, bits, int(sym), flags, search[0], search[1],
                                              p("qweight"), p("qzeros"), p("scales"), p("tensor_q"), p("zeros"),
                                              _stream(dev))
        return lib.awq_quantize_groups_ex(wb.ptr, code, rows, K, gs, bits, int(sym), flags, p("qweight"), p("qzeros"),
                                          p("scales"), p("tensor_q"), p("zeros"), _stream(dev))
    c.build()
    return c, wb, launch


def _run_quant(dev, dtype, shape, gs, bits, sym, predicate, *, skew=0, search=None, small=False):
    from awq_quantizer import _hip
    rows, K = rows_k(shape)
    w = weights(shape, dtype, rows + K + gs + bits, const=gs)
    for outs in ("all", "packed"):
        c, wb, launch = _quant_case(dev, w, shape, gs, bits, sym, skew=skew, search=search, small=small, outs=outs)
        predicate(_hip, wb, rows, K)
        c.run(launch)


def streaming(layout, gs, bits, dtype):
    def pred(_hip, wb, rows, K):
        assert _hip.ragged_eligible(dtype, rows, K, gs) and wb.addr % 16 == 0 and layout(K, gs, bits)
    return pred


def row_segment(gs, dtype):
    def pred(_hip, wb, rows, K):
        assert not _hip.ragged_eligible(dtype, rows, K, gs) and wb.addr % 16 == 0
        assert dtype in (BF16, F16, F32) and gs <= (256 if dtype == F32 else 512)
    return pred


def generic(gs, dtype):
    def pred(_hip, wb, rows, K):
        assert dtype == F64 or gs > 512 or wb.addr % 16 != 0
    return pred


# ---------------------------------------------------------------- awq_quantize_groups_ex
STREAM_CASES = [("byte", (3, 1024), 128), ("byte", (4096,), 32), ("word", (23, 384), 128), ("pad", (5, 200), 128),
                ("pad", (3, 2120), 128)]
LAYOUT = {"byte": byte_tiles, "word": word_tiles, "pad": padded_rows}


@pytest.mark.parametrize("dtype,bits,sym", COMBOS, ids=_ids)
@pytest.mark.parametrize("layout,shape,gs", STREAM_CASES, ids=_ids)
def test_quantize_streaming(layout, shape, gs, dtype, bits, sym):
    """Byte tiles with a partial last tile and a 1-D tensor, word tiles with an odd G, padded rows
    below and above one tile per row.  (Word tiles exist for 4 bits only: an 8-bit (23, 384) takes
    byte tiles, and is asserted as such.)"""
    dev = _dev()
    if layout == "word" and bits == 8:
        layout = "byte"
    _run_quant(dev, dtype, shape, gs, bits, sym, streaming(LAYOUT[layout], gs, bits, dtype))


@pytest.mark.parametrize("dtype,bits,sym", COMBOS, ids=_ids)
@pytest.mark.parametrize("shape,gs", [((4, 250), 100), ((5, 132), 128), ((2, 1032), 512)], ids=_ids)
def test_quantize_row_segment(shape, gs, dtype, bits, sym):
    """A tail group of 50, K % 8 != 0, and the largest group size.  The row-segment kernel takes
    fp32 groups up to 256, and (2, 1032) with group size 256 is a padded-rows shape of the
    streaming kernel: the fp32 case runs (2, 1036) with group size 256 (K % 8 != 0, tail 12)."""
    dev = _dev()
    if dtype == F32 and gs == 512:
        shape, gs = (2, 1036), 256
    _run_quant(dev, dtype, shape, gs, bits, sym, row_segment(gs, dtype))


@pytest.mark.parametrize("dtype,shape,gs,skew,bits,sym",
                         [(F64, (3, 200), 64, 0, 4, False), (F64, (3, 200), 64, 0, 8, True),
                          (BF16, (2, 2088), 1024, 0, 4, True), (BF16, (2, 2088), 1024, 0, 8, False),
                          (BF16, (3, 256), 128, 2, 4, False), (BF16, (3, 256), 128, 2, 8, True)], ids=_ids)
def test_quantize_generic(dtype, shape, gs, skew, bits, sym):
    dev = _dev()
    _run_quant(dev, dtype, shape, gs, bits, sym, generic(gs, dtype), skew=skew)


@pytest.mark.parametrize("dtype,bits,sym,nan", [(BF16, 4, False, False), (F16, 8, True, False), (F16, 4, False, True)],
                         ids=_ids)
def test_quantize_small_tensor(dtype, bits, sym, nan):
    """AWQ_Q_SMALL_TENSOR, (1, 40) with group size K; the fp16 NaN case pins the path's own NaN
    scale bits."""
    dev = _dev()
    w = weights((1, 40), dtype, 40 + bits, nan=False)
    if nan:
        w[0, 17] = float("nan")
    for outs in ("all", "packed"):
        c, wb, launch = _quant_case(dev, w, (1, 40), 40, bits, sym, small=True, outs=outs)
        assert wb.addr % 16 == 0 and w.numel() == 40
        c.run(launch)


# ---------------------------------------------------------------- awq_quantize_search_ex
@pytest.mark.parametrize("dtype,shape,gs,bits,sym",
                         [(BF16, (3, 1024), 128, 4, False), (F16, (3, 1024), 128, 8, True),
                          (BF16, (23, 384), 128, 4, True), (F32, (23, 384), 128, 8, False),
                          (F16, (4, 250), 100, 4, False), (BF16, (4, 250), 100, 8, True),
                          (F64, (3, 200), 64, 4, True), (F64, (3, 200), 64, 8, False)], ids=_ids)
def test_quantize_search(dtype, shape, gs, bits, sym):
    dev = _dev()
    if dtype == F64:
        pred = generic(gs, dtype)
    elif shape[1] % gs:
        pred = row_segment(gs, dtype)
    else:
        pred = streaming(byte_tiles if byte_tiles(shape[1], gs, bits) else word_tiles, gs, bits, dtype)
    _run_quant(dev, dtype, shape, gs, bits, sym, pred, search=(4, 3))


# ---------------------------------------------------------------- awq_quantize_ragged(_search)
RAGGED_SHAPES = [(3, 1024), (23, 384), (256,), (5, 200)]


@pytest.mark.parametrize("table", [True, False], ids=["block_table", "no_table"])
@pytest.mark.parametrize("search", [None, (4, 3)], ids=["rtn", "search"])
@pytest.mark.parametrize("dtype,bits,sym", COMBOS[:3], ids=_ids)
def test_quantize_ragged(dtype, bits, sym, search, table):
    """One launch over four tensors, the last with padded rows; inputs neighbours in descriptor
    order, each output kind's buffers neighbours; the descriptors and the block table live in the
    arena too."""
    dev = _dev()
    from awq_quantizer import _hip
    lib = _lib()
    gs = 128
    ws = [weights(s, dtype, 7 + i + bits, const=gs) for i, s in enumerate(RAGGED_SHAPES)]
    rk = [rows_k(s) for s in RAGGED_SHAPES]
    want = [quant_expect(w, r, k, gs, bits, sym, search) for w, (r, k) in zip(ws, rk)]
    for (r, k) in rk:
        assert _hip.ragged_eligible(dtype, r, k, gs)
    c = Call(dev, seed=31 + bits)
    wb = [c.inp(f"w{i}", w) for i, w in enumerate(ws)]
    ob = {n: [c.out(f"{n}{i}", e[n]) for i, e in enumerate(want)]
          for n in ("qweight", "qzeros", "scales", "tensor_q", "zeros")}
    n = len(ws)
    descs_b = c.inp("descs", nbytes=80 * n, pointers=True)
    # the table's length depends on the tile count alone: plan with placeholder pointers first
    plan = [_hip.TensorDesc(w=16, rows=r, K=k) for (r, k) in rk]
    total = _hip.plan_ragged(plan, bits, gs)
    arr = (_hip.TensorDesc * n)(*plan)
    tlen = lib.awq_plan_block_tensor(arr, n, total, None, 0)
    assert tlen > 0
    table_b = c.inp("block_table", nbytes=4 * tlen, pointers=True) if table else None
    c.build()
    descs = [_hip.TensorDesc(w=wb[i].addr, rows=r, K=k, qweight=ob["qweight"][i].addr, qzeros=ob["qzeros"][i].addr,
                             scales=ob["scales"][i].addr, tensor_q=ob["tensor_q"][i].addr, zeros=ob["zeros"][i].addr)
             for i, (r, k) in enumerate(rk)]
    assert _hip.plan_ragged(descs, bits, gs) == total
    for b in wb:
        assert b.addr % 16 == 0
    flags = _hip.ragged_flags(descs, gs)
    assert flags == 1                                                # AWQ_RAGGED_PADDED: (5, 200)
    arr = (_hip.TensorDesc * n)(*descs)
    descs_b.data = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    if table:
        host = torch.empty(tlen, dtype=torch.int32)
        assert host.data_ptr() % 16 == 0
        assert lib.awq_plan_block_tensor(arr, n, total, ctypes.c_void_p(host.data_ptr()), tlen) == tlen
        table_b.data = _bytes(host)
    code = _hip.AWQ_DTYPE[dtype]
    tp = table_b.ptr if table else None

    def launch():
        if search is not None:
            return lib.awq_quantize_ragged_search(descs_b.ptr, n, total, tp, code, bits, int(sym), gs, flags,
                                                  search[0], search[1], _stream(dev))
        return lib.awq_quantize_ragged(descs_b.ptr, n, total, tp, code, bits, int(sym), gs, flags, _stream(dev))
    c.run(launch)


# ---------------------------------------------------------------- awq_group_params_ex
@pytest.mark.parametrize("which", ["both", "scales", "zeros"])
@pytest.mark.parametrize("flags", [0, 1], ids=["cpu", "torch_gpu"])
@pytest.mark.parametrize("dtype,bits,sym", [(BF16, 4, False), (F64, 8, True), (F64, 4, False), (BF16, 8, True)],
                         ids=_ids)
def test_group_params(dtype, bits, sym, flags, which):
    dev = _dev()
    from awq_quantizer import _hip
    rows, K, gs = 3, 200, 64
    assert K % gs != 0                                              # a tail group of 8
    w = weights((rows, K), dtype, 5 + bits, nan=False, const=gs)
    s, z = orc.group_params(w, rows, K, gs, bits, sym, device="cuda" if flags else "cpu")
    c = Call(dev, seed=bits + flags)
    wb = c.inp("w", w)
    sb = c.out("scales", s) if which != "zeros" else None
    zb = c.out("zeros", z) if which != "scales" else None
    c.build()
    c.run(lambda: _lib().awq_group_params_ex(wb.ptr, _hip.AWQ_DTYPE[dtype], rows, K, gs, bits, int(sym), flags,
                                             sb.ptr if sb else None, zb.ptr if zb else None, _stream(dev)))


# ---------------------------------------------------------------- awq_apply_params / _ex
@pytest.mark.parametrize("gs", [64, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype,bits,sym", [(BF16, 4, False), (F16, 8, True), (F32, 4, True), (F64, 8, False)],
                         ids=_ids)
def test_apply_params(dtype, bits, sym, mode, gs):
    dev = _dev()
    from awq_quantizer import _hip
    rows, K = 3, 200
    qmin, qmax = orc.qrange(bits, sym)
    w = weights((rows, K), dtype, 9 + bits, nan=False)
    if gs == 1:          # one parameter per element: values of the dtype, not the degenerate one-element groups
        g = torch.Generator().manual_seed(bits)
        s = (torch.rand(rows, K, generator=g) * 0.01 + 1e-3).to(dtype).double()
        z = torch.randint(qmin, qmax + 1, (rows, K), generator=g).double()
    else:
        s, z = orc.group_params(w, rows, K, gs, bits, sym)
    x = w if mode == 0 else orc.apply_params(w, rows, K, gs, s, z, qmin, qmax, 0)
    want = orc.apply_params(x, rows, K, gs, s, z, qmin, qmax, mode)
    c = Call(dev, seed=bits + mode + gs)
    xb, sb, zb = c.inp("x", x), c.inp("scales", s), c.inp("zeros", z)
    ob = c.out("out", want)
    c.build()
    c.run(lambda: _lib().awq_apply_params(xb.ptr, _hip.AWQ_DTYPE[dtype], rows, K, gs, sb.ptr, zb.ptr, qmin, qmax, mode,
                                          ob.ptr, _stream(dev)))


@pytest.mark.parametrize("gs", [64, 1])
def test_apply_params_ex_int32_with_fp16_ops(gs):
    """quantize()'s int32 tensor_q dequantized with fp16 parameters: mode 1, both ops fp16."""
    dev = _dev()
    from awq_quantizer import _hip
    rows, K = 3, 200
    G = -(-K // gs)
    g = torch.Generator().manual_seed(gs)
    x = torch.randint(-8, 8, (rows, K), generator=g, dtype=torch.int32)
    s16 = (torch.rand(rows, G, generator=g) * 0.01 + 1e-3).to(F16)
    z16 = torch.randint(-8, 8, (rows, G), generator=g).to(F16)
    col = torch.arange(K) // gs
    want = orc.apply_promoted(x, s16[:, col].contiguous(), z16[:, col].contiguous(), -8, 7, 1, False)
    assert want.dtype == F16 and want.shape == (rows, K)
    c = Call(dev, seed=gs)
    xb, sb, zb = c.inp("x", x), c.inp("scales", s16.double()), c.inp("zeros", z16.double())
    ob = c.out("out", want)
    c.build()
    c.run(lambda: _lib().awq_apply_params_ex(xb.ptr, _hip.APPLY_DTYPE[I32], rows, K, gs, sb.ptr, zb.ptr, -8, 7, 1,
                                             _hip.APPLY_OP_DTYPE[F16], _hip.APPLY_OP_DTYPE[F16], 0, ob.ptr,
                                             _stream(dev)))


# ---------------------------------------------------------------- awq_dequantize(_packed), awq_pack_rows
DQ_SHAPES = [((3, 1024), 128), ((5, 200), 128), ((4, 250), 100)]


def _masked(t, bits, qmin):
    """The values the packed fields hold ((v - qmin) mod 2^bits + qmin)."""
    return (((t.long() - qmin) & ((1 << bits) - 1)) + qmin).to(I32)


@pytest.mark.parametrize("skew", [0, 4])
@pytest.mark.parametrize("packed", [False, True], ids=["int32", "packed"])
@pytest.mark.parametrize("bits,sym,dtype", [(4, False, BF16), (8, True, F16)], ids=_ids)
@pytest.mark.parametrize("shape,gs", DQ_SHAPES, ids=_ids)
def test_dequantize(shape, gs, bits, sym, dtype, packed, skew):
    """(5, 200): a tail group of 72 (n % 8 == 0 with n < group size); (4, 250): tail 50 (n % 8 = 2,
    the 0x7FFFFFFF rule); a NaN group in every input."""
    dev = _dev()
    rows, K = shape
    qmin = orc.qrange(bits, sym)[0]
    w = weights(shape, dtype, rows + K + bits, const=gs)
    tq, sc, zp = orc.quantize_groups(w, rows, K, gs, bits, sym)
    tq = tq.reshape(rows, K)
    if packed:
        tq, zp = _masked(tq, bits, qmin), _masked(zp, bits, qmin)
    want = orc.dequantize({"tensor_q": tq, "scales": sc, "zero_points": zp, "group_size": torch.tensor(gs)})
    assert bool(torch.isnan(want).any()) and K % gs in ((0,) if shape == (3, 1024) else (72, 50))
    c = Call(dev, seed=K + bits + skew)
    if packed:
        qb, zb = c.inp("qweight", orc.pack_rows(tq, bits, qmin)), c.inp("qzeros", orc.pack_rows(zp, bits, qmin))
    else:
        qb, zb = c.inp("tensor_q", tq), c.inp("zeros", zp)
    sb = c.inp("scales", sc)
    ob = c.out("out", want, skew=skew)
    c.build()
    assert ob.addr % 16 == skew
    if packed:
        c.run(lambda: _lib().awq_dequantize_packed(qb.ptr, zb.ptr, sb.ptr, rows, K, gs, bits, int(sym), ob.ptr,
                                                   _stream(dev)))
    else:
        c.run(lambda: _lib().awq_dequantize(qb.ptr, sb.ptr, zb.ptr, rows, K, gs, ob.ptr, _stream(dev)))


@pytest.mark.parametrize("bits,qmin", [(4, 0), (4, -8), (8, 0), (8, -128)])
@pytest.mark.parametrize("n", [8, 9, 1000])
def test_pack_rows(n, bits, qmin):
    dev = _dev()
    rows = 3
    g = torch.Generator().manual_seed(n + bits)
    v = torch.randint(qmin, qmin + (1 << bits), (rows, n), generator=g, dtype=torch.int32)
    v[0, 0] = -2 ** 31                                              # a NaN element's value
    c = Call(dev, seed=n + bits)
    vb = c.inp("v", v)
    ob = c.out("packed", orc.pack_rows(v, bits, qmin))
    c.build()
    c.run(lambda: _lib().awq_pack_rows(vb.ptr, rows, n, bits, qmin, ob.ptr, _stream(dev)))


# ---------------------------------------------------------------- awq_export_autoawq_gemm
@pytest.mark.parametrize("N,K,gs,skew,sym", [(8, 128, 128, 0, False), (72, 512, 64, 0, True), (264, 288, 32, 0, False),
                                             (24, 264, 8, 0, True), (72, 512, 64, 2, False)], ids=_ids)
def test_export_autoawq_gemm(N, K, gs, skew, sym):
    """G = 8 with aligned scales: the vector group kernel; G = 9, G = 33 and the skewed scales_t:
    the scalar one; K % 32 == 0: 16-B qweight loads, else 4-B loads; (264, 288) crosses both
    qweight tile edges.  (The export pairs row n with row n + 1: N - 1 is the last pair's second.)"""
    dev = _dev()
    G = K // gs
    vec_group = G % 8 == 0 and skew == 0
    assert vec_group == ((N, K, gs, skew) == (72, 512, 64, 0))
    assert (K % 32 == 0) == (K != 264) and N % 8 == 0 and K % gs == 0
    qmin = orc.qrange(4, sym)[0]
    w = weights((N, K), BF16, N + K, nan=False)
    tq, sc, zp = orc.quantize_groups(w, N, K, gs, 4, sym)
    tq = tq.reshape(N, K)
    qw_t, qz_t, sc_t = orc.autoawq_pack(tq.long() - qmin, zp.long() - qmin, sc)
    c = Call(dev, seed=N + K + skew)
    qb = c.inp("qweight", orc.pack_rows(tq, 4, qmin))
    zb = c.inp("qzeros", orc.pack_rows(zp, 4, qmin))
    sb = c.inp("scales", sc)
    oq, oz = c.out("qweight_t", qw_t), c.out("qzeros_t", qz_t)
    os_ = c.out("scales_t", sc_t, skew=skew)
    c.build()
    assert qb.addr % 16 == 0 and sb.addr % 16 == 0 and os_.addr % 16 == skew
    c.run(lambda: _lib().awq_export_autoawq_gemm(qb.ptr, zb.ptr, sb.ptr, N, K, gs, 4, oq.ptr, oz.ptr, os_.ptr,
                                                 _stream(dev)))


# ---------------------------------------------------------------- awq_quant_error
@pytest.mark.parametrize("totals", [True, False], ids=["totals", "no_totals"])
@pytest.mark.parametrize("dtype,bits,sym", COMBOS[:3], ids=_ids)
@pytest.mark.parametrize("shape,gs", DQ_SHAPES, ids=_ids)
def test_quant_error(shape, gs, dtype, bits, sym, totals):
    """(3, 1024) gs 128: the streaming kernel; tail groups: one wave per group."""
    dev = _dev()
    from awq_quantizer import _hip
    lib = _lib()
    rows, K = shape
    G = -(-K // gs)
    qmin = orc.qrange(bits, sym)[0]
    w = weights(shape, dtype, rows + K + bits, const=gs)
    ref = orc.quantize(w, bits=bits, group_size=gs, symmetric=sym)
    e = expect_qerror(w, ref)
    stats = np.stack([e[k].reshape(-1) for k in ("group_abs", "group_sq", "group_w_sq", "group_max")])
    assert stats.shape == (4, rows * G) and stats.dtype == np.float32
    nbytes = lib.awq_quant_error_work_bytes(rows, K, gs)
    assert nbytes >= 0 and nbytes % 8 == 0
    c = Call(dev, seed=K + bits)
    wb = c.inp("w", w)
    qb = c.inp("qweight", orc.pack_rows(ref["tensor_q"].reshape(rows, K), bits, qmin))
    zb = c.inp("qzeros", orc.pack_rows(ref["zero_points"], bits, qmin))
    sb = c.inp("scales", ref["scales"])
    gb = c.out("group_stats", stats)
    nb = c.out("group_nonfinite", e["group_nonfinite"].reshape(-1).astype(np.int32))
    kb = c.work("work", nbytes) if totals and nbytes else None
    tb = c.out("totals", e["totals"]) if totals else None
    c.build()
    assert (K % gs == 0 and wb.addr % 16 == 0 and qb.addr % 16 == 0) == (shape == (3, 1024))
    c.run(lambda: lib.awq_quant_error(wb.ptr, _hip.AWQ_DTYPE[dtype], rows, K, gs, bits, int(sym), qb.ptr, zb.ptr,
                                      sb.ptr, gb.ptr, nb.ptr, kb.ptr if kb else None, tb.ptr if tb else None,
                                      _stream(dev)))


# ---------------------------------------------------------------- activation-aware search
def _acts(T, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, K, generator=g) * 3).to(dtype)


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=_ids)
@pytest.mark.parametrize("K", [8, 264])
@pytest.mark.parametrize("T", [1, 33, 257])
def test_act_stats(T, K, dtype):
    dev = _dev()
    from awq_quantizer import _hip
    x = _acts(T, K, dtype, T + K)
    xm, xs = orc.act_stats(x)
    c = Call(dev, seed=T + K)
    xb = c.inp("x", x)
    kb = c.work("work", 8 * 2 * (-(-T // 256)) * K)
    mb, sb = c.out("x_mean", xm), c.out("x_sq", xs)
    c.build()
    c.run(lambda: _lib().awq_act_stats(xb.ptr, _hip.AWQ_DTYPE[dtype], T, K, kb.ptr, mb.ptr, sb.ptr, _stream(dev)))


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=_ids)
@pytest.mark.parametrize("gs", [128, 16], ids=["one_pass", "two_pass"])
def test_weight_colsum_and_column_mean(gs, dtype):
    """Two linears (1 and 257 rows: one block, and a full block plus a one-row block) write their
    slices of one neighbouring `partial`; gmax_work is exact for the two-pass path and handed to
    the one-pass path as well."""
    dev = _dev()
    from awq_quantizer import _hip
    lib = _lib()
    K, rows = 256, (1, 257)
    assert (gs in (32, 64, 128, 256)) == (gs == 128) and K % gs == 0
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
    code = _hip.AWQ_DTYPE[dtype]

    def launch():
        off = 0
        for w, b, gw, nb in zip(ws, wb, gb, nblk):
            assert b.addr % 16 == 0
            rc = lib.awq_weight_colsum(b.ptr, code, w.shape[0], K, gs, gw.ptr, pb.at(8 * off * K), _stream(dev))
            if rc:
                return rc
            off += nb
        return lib.awq_column_mean(pb.ptr, sum(nblk), K, float(sum(rows)), ob.ptr, _stream(dev))
    c.run(launch)


@pytest.mark.parametrize("duo", [False, True], ids=["no_w_mean", "w_mean"])
@pytest.mark.parametrize("n_grid", [1, 5])
@pytest.mark.parametrize("K", [8, 264])
def test_act_scale_and_recip_tables(K, n_grid, duo):
    """awq_act_scale_table, awq_act_scale_table_ws (work exact) and awq_act_recip_table (the
    header's definition: RN_f32(1 / table), every entry in range here) in one arena."""
    dev = _dev()
    lib = _lib()
    g = torch.Generator().manual_seed(K + n_grid)
    xm = torch.exp2(torch.rand(K, generator=g) * 8 - 4).float()
    wm = torch.exp2(torch.rand(K, generator=g) * 8 - 4).float() if duo else None
    table = orc.act_scale_table(xm, wm, n_grid)
    assert bool(((table > 2.0 ** -60) & (table < 2.0 ** 60)).all())
    recip = torch.ones((), dtype=F32) / table
    c = Call(dev, seed=K + n_grid + duo)
    xb = c.inp("x_mean", xm)
    mb = c.inp("w_mean", wm) if duo else None
    t1 = c.out("table", table)
    kb = c.work("work", 8 * n_grid * (K + 3 * (-(-K // 256))))
    t2 = c.out("table_ws", table)
    tin = c.inp("table_in", table)
    rb = c.out("rtable", recip)
    c.build()
    mp = mb.ptr if duo else None

    def launch():
        return (lib.awq_act_scale_table(xb.ptr, mp, K, n_grid, t1.ptr, _stream(dev))
                or lib.awq_act_scale_table_ws(xb.ptr, mp, K, n_grid, kb.ptr, t2.ptr, _stream(dev))
                or lib.awq_act_recip_table(tin.ptr, n_grid, K, rb.ptr, _stream(dev)))
    c.run(launch)


@pytest.mark.parametrize("rtable", [True, False], ids=["rtable", "ieee"])
@pytest.mark.parametrize("dtype,gs,bits,sym", [(BF16, 8, 4, False), (F16, 128, 8, True), (F32, 512, 4, True),
                                               (BF16, 128, 4, True), (F16, 8, 8, False), (BF16, 512, 8, False)],
                         ids=_ids)
def test_act_search_losses(dtype, gs, bits, sym, rtable):
    """Two linears (3 and 5 rows) write one `part` at their offsets, part_stride exactly the total.
    K = 256, and 512 for group size 512 (the entry point takes K % group_size == 0 only)."""
    dev = _dev()
    from awq_quantizer import _hip
    lib = _lib()
    K, n_grid = max(256, gs), 5
    assert K % gs == 0
    ws = [weights((r, K), dtype, r + gs, nan=False, scale=0.02) for r in (3, 5)]
    g = torch.Generator().manual_seed(gs + bits)
    xm = torch.exp2(torch.rand(K, generator=g) * 6 - 3).float()
    xs = (torch.rand(K, generator=g) ** 4 + 1e-4).float()
    table = orc.act_scale_table(xm, None, n_grid)
    _, _, part = orc.act_search_losses(ws, xs, table, gs, bits, sym)
    groups = [w.shape[0] * (K // gs) for w in ws]
    stride = sum(groups)
    assert part.shape == (n_grid, stride) and not bool(torch.isnan(part).any())
    c = Call(dev, seed=gs + bits)
    wb = [c.inp(f"w{i}", w) for i, w in enumerate(ws)]
    tb, xb = c.inp("table", table), c.inp("x_sq", xs)
    rb = c.inp("rtable", torch.ones((), dtype=F32) / table) if rtable else None
    pb = c.out("part", part)
    c.build()
    code = _hip.AWQ_DTYPE[dtype]

    def launch():
        off = 0
        for w, b, ng in zip(ws, wb, groups):
            rc = lib.awq_act_search_losses(b.ptr, code, w.shape[0], K, gs, bits, int(sym), tb.ptr,
                                           rb.ptr if rb else None, n_grid, xb.ptr, pb.at(4 * off), stride, _stream(dev))
            if rc:
                return rc
            off += ng
        return 0
    c.run(launch)


@pytest.mark.parametrize("drop", [None, "losses", "best", "s_best"])
@pytest.mark.parametrize("n_grid", [1, 5])
@pytest.mark.parametrize("stride", [1, 65, 1025])
def test_act_search_select(stride, n_grid, drop):
    dev = _dev()
    K = 24
    g = torch.Generator().manual_seed(stride + n_grid)
    part = (torch.rand(n_grid, stride, generator=g) *
            torch.exp2(torch.randint(-20, 20, (n_grid, stride), generator=g).float())).float()
    table = torch.rand(n_grid, K, generator=g).float()
    losses, best = orc.act_search_select(part)
    c = Call(dev, seed=stride + n_grid)
    pb, tb = c.inp("part", part), c.inp("table", table)
    kb = c.work("work", 8 * n_grid * (-(-stride // 1024)))
    lb = c.out("losses", losses) if drop != "losses" else None
    bb = c.out("best", torch.tensor([best], dtype=I32)) if drop != "best" else None
    sb = c.out("s_best", table[best]) if drop != "s_best" else None
    c.build()
    q = lambda b: b.ptr if b else None
    c.run(lambda: _lib().awq_act_search_select(pb.ptr, n_grid, stride, tb.ptr, K, kb.ptr, q(lb), q(bb), q(sb),
                                               _stream(dev)))


@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "skewed"])
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=_ids)
def test_apply_input_scale(dtype, skew):
    """(3, 264); skewed: w and out one element off 16-B alignment."""
    dev = _dev()
    from awq_quantizer import _hip
    rows, K = 3, 264
    w = weights((rows, K), dtype, 264, nan=False)
    s = torch.exp2(torch.rand(K, generator=torch.Generator().manual_seed(3)) * 4 - 2).float()
    c = Call(dev, seed=K + skew)
    wb = c.inp("w", w, skew=skew * ESIZE[dtype])
    sb = c.inp("s", s)
    ob = c.out("out", orc.apply_input_scale(w, s), skew=skew * ESIZE[dtype])
    c.build()
    assert (wb.addr % 16 == 0) == (skew == 0) and (ob.addr % 16 == 0) == (skew == 0)
    c.run(lambda: _lib().awq_apply_input_scale(wb.ptr, _hip.AWQ_DTYPE[dtype], rows, K, sb.ptr, ob.ptr, _stream(dev)))


@pytest.mark.parametrize("dtype,bits,sym", COMBOS, ids=_ids)
@pytest.mark.parametrize("shape", [(3, 1024), (23, 384)], ids=_ids)
def test_quantize_groups_scaled(shape, dtype, bits, sym):
    dev = _dev()
    from awq_quantizer import _hip
    rows, K = shape
    gs = 128
    assert _hip.scaled_eligible(dtype, rows, K, gs)
    w = weights(shape, dtype, rows + bits, const=gs)
    s = torch.exp2(torch.rand(K, generator=torch.Generator().manual_seed(K)) * 4 - 2).float()
    want = quant_expect(orc.apply_input_scale(w, s), rows, K, gs, bits, sym)
    c = Call(dev, seed=K + bits)
    wb, sb = c.inp("w", w), c.inp("col_scale", s)
    ob = [c.out(n, want[n]) for n in ("qweight", "qzeros", "scales")]
    c.build()
    assert wb.addr % 16 == 0 and sb.addr % 16 == 0
    c.run(lambda: _lib().awq_quantize_groups_scaled(wb.ptr, _hip.AWQ_DTYPE[dtype], rows, K, gs, bits, int(sym), sb.ptr,
                                                    ob[0].ptr, ob[1].ptr, ob[2].ptr, _stream(dev)))


# ---------------------------------------------------------------- awq_quantize_clip_scaled
CLIP_CASES = [  # name, shape, gs, w skew (elements), loss slack, outputs
    ("streaming", (3, 1024), 128, 0, 0, "all"),
    ("zeroed_qzeros", (23, 384), 128, 0, 0, "all"),
    ("per_group", (4, 256), 16, 0, 0, "all"),
    ("fallback", (3, 1024), 128, 1, 0, "all"),
    ("loss_slack", (3, 1024), 128, 0, 37, "all"),
    ("loss_only", (23, 384), 128, 0, 0, "loss")]


@pytest.mark.parametrize("dtype,bits,sym", COMBOS[:3], ids=_ids)
@pytest.mark.parametrize("name,shape,gs,wskew,slack,outs", CLIP_CASES, ids=_ids)
def test_quantize_clip_scaled(name, shape, gs, wskew, slack, outs, dtype, bits, sym):
    """n_grid 20, n_candidates 10.  zeroed_qzeros: G % (32 / bits) != 0, the streaming kernel ORs
    shared qzeros words into memory the entry point zeroes first — here it starts from the fill;
    loss_slack: loss_stride = rows G + 37, the slack of both rows must keep the fill."""
    dev = _dev()
    from awq_quantizer import _hip
    rows, K = shape
    G = K // gs
    n = rows * G
    w = weights(shape, dtype, rows + K + bits, const=gs)
    g = torch.Generator().manual_seed(K + gs)
    s = torch.exp2(torch.rand(K, generator=g) * 4 - 2).float()
    xs = (torch.rand(K, generator=g) ** 4 + 1e-4).float()
    want = expect_clip(w, s, xs, gs, bits, sym, 20, 10)
    stride = n + slack
    loss = np.zeros((2, stride), dtype=np.float32)
    loss[:, :n] = want["loss"]
    owned = torch.zeros((2, stride), dtype=torch.bool)
    owned[:, :n] = True
    c = Call(dev, seed=K + gs + bits)
    wb = c.inp("w", w, skew=wskew * ESIZE[dtype])
    sb, xb = c.inp("col_scale", s), c.inp("x_sq", xs)
    rb = c.inp("col_rscale", torch.ones((), dtype=F32) / s) if name != "per_group" else None
    ob = {k: c.out(k, want[k]) for k in ("qweight", "qzeros", "scales")} if outs == "all" else {}
    bb = c.out("best_idx", want["best_idx"].to(I32))
    lb = c.out("group_loss", loss, nan_dtype=F32, written=elem_mask(owned, 4))
    c.build()
    stream_path = gs in (32, 64, 128, 256) and wb.addr % 16 == 0 and sb.addr % 16 == 0 and xb.addr % 16 == 0
    assert stream_path == (name not in ("per_group", "fallback"))
    if name in ("zeroed_qzeros", "loss_only"):
        assert G % (32 // bits) != 0
    p = lambda k: ob[k].ptr if k in ob else None
    c.run(lambda: _lib().awq_quantize_clip_scaled(wb.ptr, _hip.AWQ_DTYPE[dtype], rows, K, gs, bits, int(sym), sb.ptr,
                                                  rb.ptr if rb else None, xb.ptr, 20, 10, p("qweight"), p("qzeros"),
                                                  p("scales"), bb.ptr, lb.ptr, stride, _stream(dev)))


# ---------------------------------------------------------------- awq_fold_rows
FOLD_CASES = [((3, 1024), 0, False), ((5, 264), 0, False), ((2, 2056), 0, False), ((7, 1), 0, False),
              ((3, 13), 0, False), ((3, 1024), 1, False), ((5, 264), 0, True), ((3, 13), 0, True)]


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=_ids)
@pytest.mark.parametrize("shape,skew,in_place", FOLD_CASES, ids=_ids)
def test_fold_rows(shape, skew, in_place, dtype):
    """Streaming structure (16-B aligned, K % 8 == 0: one row per tile, several rows per tile,
    K >= 2048), one element per lane (K = 1, K = 13, an `out` one element off alignment), and
    out == w (the expectation comes from a copy; the input is then not marked untouched)."""
    dev = _dev()
    from awq_quantizer import _hip
    rows, K = shape
    w = weights(shape, dtype, rows + K, nan=False)
    s = torch.exp2(torch.rand(rows, generator=torch.Generator().manual_seed(rows)) * 4 - 2).float()
    want = (w.clone().float() / s[:, None]).to(dtype)
    c = Call(dev, seed=rows + K + skew)
    if in_place:
        wb = ob = c.inp("w_out", w, untouched=False, expect=want)
    else:
        wb = c.inp("w", w)
    sb = c.inp("row_scale", s)
    if not in_place:
        ob = c.out("out", want, skew=skew * ESIZE[dtype])
    c.build()
    assert (wb.addr % 16 == 0 and ob.addr % 16 == 0 and K % 8 == 0) == (K % 8 == 0 and skew == 0)
    c.run(lambda: _lib().awq_fold_rows(wb.ptr, _hip.AWQ_DTYPE[dtype], rows, K, sb.ptr, ob.ptr, _stream(dev)))


# ---------------------------------------------------------------- measurement helpers
def _words(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(I32)


@pytest.mark.parametrize("n", [16, 4096, 4096 * 8 * 3 + 48])
def test_stream_copy(n):
    dev = _dev()
    src = _words(n // 4, n)
    c = Call(dev, seed=n)
    sb = c.inp("src", src)
    db = c.out("dst", src)
    c.build()
    c.run(lambda: _lib().awq_stream_copy(sb.ptr, db.ptr, n, _stream(dev)))


@pytest.mark.parametrize("n", [4096, 4096 * 8 * 3 + 4096])
def test_stream_ceiling(n):
    dev = _dev()
    src = _words(n // 4, n)
    q = src.view(-1, 4, 256)
    c = Call(dev, seed=n)
    sb = c.inp("src", src)
    db = c.out("dst", (q[:, 0] ^ q[:, 1] ^ q[:, 2] ^ q[:, 3]).contiguous())
    c.build()
    assert db.nbytes == n // 4
    c.run(lambda: _lib().awq_stream_ceiling(sb.ptr, db.ptr, n, _stream(dev)))


@pytest.mark.parametrize("n_out", [16, 4096, 1 << 20, (1 << 20) + 48])
def test_dequant_ceiling(n_out):
    dev = _dev()
    quads = n_out // 4
    words = _words(-(-quads // 2), n_out)
    w = words.to(torch.int64) & 0xFFFFFFFF
    q = torch.arange(quads)
    half = (w[q // 2] >> (16 * (q % 2))) & 0xFFFF
    want = torch.stack([((half >> (4 * j)) & 15).float() for j in range(4)], dim=1).reshape(-1)
    c = Call(dev, seed=n_out % 1000)
    wb = c.inp("words", words)
    ob = c.out("out", want)
    c.build()
    assert wb.nbytes * 8 >= ob.nbytes and wb.nbytes == 4 * (-(-n_out // 8))
    c.run(lambda: _lib().awq_dequant_ceiling(wb.ptr, ob.ptr, 4 * n_out, _stream(dev)))
