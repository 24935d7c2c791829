"""awq_export_gptq / awq_import_gptq (csrc/awq_gptq.hip) and AWQQuantizer.export_gptq / import_gptq /
dequantize_gptq on the GPU, against the CPU restatement of the layout (tests/gptq_layout.py).

Shapes.  The kernels transpose 64 x 64 tiles (32-bit words of qweight: N x K/8; fp16 scales:
N x G) and gather qzeros in blocks of 64 (N/8) x 4 (ceil(G/8)) words.  SHAPES is the issue's set: one
word row; G = 1, 5, 9 (a ragged last qzeros word); N = 8 .. 1032 and K/8 = 4 .. 144 on both sides
of the 64 edge and beyond two tiles; N/8 = 65, 129 beyond one qzeros block.  EXTRA adds what that
set leaves out for this tiling: (136, 2048, 32) has G = 64, the only G % 8 == 0, which the 16-B
scale path needs; (72, 2080, 32) has G = 65, scales beyond one tile along G and ceil(G/8) = 9 > 4,
a second and third qzeros block along G; (16, 72, 8) has K/8 = 9, K % 32 != 0: the 4-B word path
on aligned pointers.  The grids are not capped (one workgroup per tile), so there is no diag cap
to test.  Every case's quantize result is computed once and shared.
"""
import pytest
import torch

import gptq_layout as gl
from test_gpu_bounds import BF16, F16, F32, Call, _dev, _lib, _stream

pytestmark = pytest.mark.gpu

SHAPES = [(8, 32, 32), (8, 128, 128), (72, 160, 32), (136, 288, 32), (264, 576, 64), (520, 1152, 128), (1032, 64, 64)]
EXTRA = [(136, 2048, 32), (72, 2080, 32), (16, 72, 8)]
FORMATS = {"gptq": 1, "gptq_v2": 0}
_ids = lambda v: str(v).replace("torch.", "")
_REF = {}


def quantizer(gs, sym=False):
    from awq_quantizer.quantization import AWQQuantizer
    return AWQQuantizer(bits=4, group_size=gs, symmetric=sym, device="cuda:0", logger_level="ERROR")


def crafted(N, K, gs, dtype):
    """randn x 0.02 whose rows 0, 1, 2 start with a group spanning [0, 15/16], [-15/16, 0] and
    [-1/16, 14/16] (scale 1/16 exactly: asymmetric zero points 0, 15 and 1) and whose row 3 starts
    with a group spanning [-15/16, 15/16] (symmetric scale 1/8 exactly: -15/16 is q = -7.5 -> -8,
    15/16 is 7.5 -> 8, clamped to 7)."""
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(N * 3 + K + gs)) * 0.02
    for row, (lo, hi) in enumerate(((0.0, 0.9375), (-0.9375, 0.0), (-0.0625, 0.875), (-0.9375, 0.9375))):
        w[row, :gs] = torch.linspace(lo, hi, gs)
    return w.to(dtype)


def packed(N, K, gs, dtype, sym):
    """(quantize_packed(crafted weight) on the device, its CPU copy), once per case."""
    key = (N, K, gs, dtype, sym)
    if key not in _REF:
        p = quantizer(gs, sym).quantize_packed(crafted(N, K, gs, dtype).to("cuda:0"))
        _REF[key] = (p, {k: v.cpu() for k, v in p.items()})
    return _REF[key]


def bits16(t):
    return t.cpu().contiguous().view(torch.int16)


def same(got, want, what=""):
    for k in ("qweight", "qzeros", "g_idx"):
        if k in want:
            assert torch.equal(got[k].cpu(), want[k]), f"{what} {k}"
    assert torch.equal(bits16(got["scales"]), bits16(want["scales"])), f"{what} scales"


# ---------------------------------------------------------------- against the helper
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=_ids)
@pytest.mark.parametrize("N,K,gs", SHAPES + EXTRA, ids=_ids)
def test_export_round_trip_and_dequantize(N, K, gs, dtype, sym, fmt):
    """export == the helper on the packed result; import(export(p)) == p word for word (the pad
    fields of a ragged last qzeros word 0, as quantize writes them); the published GPTQ formula on
    the exported tensors == awq_dequantize_packed, bit for bit."""
    _dev()
    off = FORMATS[fmt]
    p, pc = packed(N, K, gs, dtype, sym)
    G = K // gs
    # the crafted fields are really there
    u, z = gl.fields_of(pc["qweight"], K), gl.fields_of(pc["qzeros"], G)
    assert int(u.min()) == 0 and int(u.max()) == 15                  # q = 0 and 15 (symmetric: -8 and 7)
    if sym:
        assert bool((z == 8).all()) and int(u[3, 0]) == 0 and int(u[3, gs - 1]) == 15
    else:
        assert [int(z[r, 0]) for r in range(3)] == [0, 15, 1]
    q = quantizer(gs, sym)
    got = q.export_gptq(p, fmt)
    want = gl.from_packed(pc, off)
    assert got["qweight"].is_cuda and got["qweight"].shape == (K // 8, N) and got["qzeros"].shape == (G, N // 8)
    assert got["scales"].shape == (G, N) and got["g_idx"].shape == (K,) and got["g_idx"].dtype == torch.int32
    same(got, want, "export")
    assert int(got["zero_points_at_0"]) == (int((z == 0).sum()) if off else 0)
    if sym:
        assert int(got["zero_points_at_0"]) == 0
        stored = (8 - off) * 0x11111111
        assert bool((got["qzeros"].cpu() == (stored - (1 << 32) if stored >= 1 << 31 else stored)).all())
    elif off:                                                        # v1 stores zero points 0, 1, 15 as 15, 0, 14
        assert [int(want["qzeros"][0, 0]) >> (4 * r) & 15 for r in range(3)] == [15, 14, 0]
    r = q.import_gptq({k: got[k] for k in ("qweight", "qzeros", "scales", "g_idx")}, checkpoint_format=fmt)
    same(r, pc, "import")
    for k in ("bits", "group_size", "symmetric", "shape"):
        assert torch.equal(r[k], pc[k]) and r[k].dtype == pc[k].dtype, k
    dq = gl.dequantize({k: got[k].cpu() for k in ("qweight", "qzeros", "scales", "g_idx")}, off)
    ref = q.dequantize_packed(p).cpu()
    assert torch.equal(dq.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(q.dequantize_gptq(got, checkpoint_format=fmt).cpu().view(torch.int32), ref.view(torch.int32))


def test_export_takes_the_weight_itself():
    _dev()
    N, K, gs = 72, 160, 32
    p, pc = packed(N, K, gs, BF16, False)
    got = quantizer(gs).export_gptq(crafted(N, K, gs, BF16).to("cuda:0"))
    same(got, gl.from_packed(pc, 1))


def test_import_on_random_words():
    """Not only what quantize produces: any 32-bit words, any fp16 bits."""
    _dev()
    N, K, gs = 136, 288, 32
    G = K // gs
    g = torch.Generator().manual_seed(11)
    rnd = lambda *sh: torch.randint(-2 ** 31, 2 ** 31, sh, generator=g, dtype=torch.int64).to(torch.int32)
    t = {"qweight": rnd(K // 8, N), "qzeros": rnd(G, N // 8),
         "scales": torch.randint(-2 ** 15, 2 ** 15, (G, N), generator=g, dtype=torch.int16).view(torch.float16)}
    for fmt, off in FORMATS.items():
        r = quantizer(gs).import_gptq(t, checkpoint_format=fmt)
        same(r, gl.to_packed_words(t, off), fmt)
        back = quantizer(gs).export_gptq(r, fmt)
        same(back, t, fmt + " back")


# ---------------------------------------------------------------- paths and optional outputs
def _raw(dev, p, N, K, gs, off, sym, shift):
    """Both entries through _hip on buffers whose every pointer is 16-B aligned (shift 0) or 4 B past
    it (shift 1 word); -> the seven outputs on the CPU."""
    from awq_quantizer import _hip
    G = K // gs

    def place(t):
        flat = t.contiguous().reshape(-1)
        n = shift * (4 // flat.element_size())
        buf = torch.empty(flat.numel() + n + 8, dtype=flat.dtype, device=dev)
        assert buf.data_ptr() % 16 == 0
        v = buf[n:n + flat.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 * shift
        return v
    ins = [place(p[k]) for k in ("qweight", "qzeros", "scales")]
    sh = {"qweight": (K // 8, N), "qzeros": (G, N // 8), "scales": (G, N), "g_idx": (K,)}
    outs = [place(torch.full(sh[k], 0x5A5A if k == "scales" else 0x5A5A5A5A,
                             dtype=torch.int16 if k == "scales" else torch.int32, device=dev)) for k in sh]
    outs[2] = outs[2].view(torch.float16)
    _hip.export_gptq(*ins, N, K, gs, 4, sym, off, *outs)
    back = [place(torch.full_like(p[k], 0x5A)) for k in ("qweight", "qzeros", "scales")]
    _hip.import_gptq(*outs[:3], N, K, gs, 4, sym, off, *back)
    return [bits16(t) if t.dtype == torch.float16 else t.cpu() for t in outs + back]


@pytest.mark.parametrize("N,K,gs", [(136, 2048, 32), (264, 576, 64)], ids=_ids)
def test_wide_and_element_paths_give_the_same_bits(N, K, gs):
    """16-B aligned pointers with K % 32 == 0 (and, first shape, G % 8 == 0) take the 16-B
    accesses; the same buffers 4 B further on take the element path."""
    dev = _dev()
    assert K % 32 == 0 and ((K // gs) % 8 == 0) == (N == 136)
    p, pc = packed(N, K, gs, BF16, False)
    wide, elem = _raw(dev, p, N, K, gs, 1, False, 0), _raw(dev, p, N, K, gs, 1, False, 1)
    for a, b in zip(wide, elem):
        assert torch.equal(a, b)
    want = gl.from_packed(pc, 1)
    assert torch.equal(wide[0], want["qweight"]) and torch.equal(wide[1], want["qzeros"])
    assert torch.equal(wide[2], bits16(want["scales"])) and torch.equal(wide[3], want["g_idx"])
    assert torch.equal(wide[4], pc["qweight"]) and torch.equal(wide[5], pc["qzeros"])
    assert torch.equal(wide[6], bits16(pc["scales"]))


@pytest.mark.parametrize("which", ["qweight", "qzeros", "scales", "g_idx"])
def test_null_outputs(which):
    """One output only: the others are NULL, and so are their inputs (they are not looked at)."""
    dev = _dev()
    from awq_quantizer import _hip
    N, K, gs = 72, 160, 32
    G = K // gs
    p, pc = packed(N, K, gs, BF16, False)
    want = gl.from_packed(pc, 1)
    names = ("qweight", "qzeros", "scales")
    out = torch.empty_like(want[which], device=dev)
    _hip.export_gptq(*[(p[k] if k == which else None) for k in names], N, K, gs, 4, False, 1,
                     *[(out if k == which else None) for k in names + ("g_idx",)])
    view = bits16 if which == "scales" else (lambda t: t.cpu())
    assert torch.equal(view(out), view(want[which]))
    if which == "g_idx":
        return
    back = torch.empty_like(pc[which], device=dev)
    _hip.import_gptq(*[(out if k == which else None) for k in names], N, K, gs, 4, False, 1,
                     *[(back if k == which else None) for k in names])
    assert torch.equal(view(back), view(pc[which]))


# ---------------------------------------------------------------- guard bands, dirty outputs
GUARD = [(72, 160, 32, 0, False, 1), (264, 576, 64, 0, True, 1), (136, 2048, 32, 0, False, 0),
         (136, 2048, 32, 4, False, 1), (16, 72, 8, 0, False, 1)]


@pytest.mark.parametrize("N,K,gs,skew,sym,off", GUARD, ids=_ids)
def test_export_guard_bands(N, K, gs, skew, sym, off):
    """Every output exactly its size in a guard-band arena, from the fill and from its complement.
    skew 4: every pointer 4 B past 16-B alignment (the element path)."""
    dev = _dev()
    _, pc = packed(N, K, gs, BF16, sym)
    want = gl.from_packed(pc, off)
    c = Call(dev, seed=N + K + skew)
    ins = [c.inp(k, pc[k], skew=skew) for k in ("qweight", "qzeros", "scales")]
    outs = [c.out(k + "_t", want[k], skew=skew) for k in ("qweight", "qzeros", "scales", "g_idx")]
    c.build()
    assert all(b.addr % 16 == skew for b in ins + outs)
    c.run(lambda: _lib().awq_export_gptq(*[b.ptr for b in ins], N, K, gs, 4, int(sym), off, *[b.ptr for b in outs],
                                         _stream(dev)))


@pytest.mark.parametrize("N,K,gs,skew,sym,off", GUARD, ids=_ids)
def test_import_guard_bands(N, K, gs, skew, sym, off):
    dev = _dev()
    _, pc = packed(N, K, gs, BF16, sym)
    src = gl.from_packed(pc, off)
    c = Call(dev, seed=N + K + skew + 1)
    ins = [c.inp(k + "_t", src[k], skew=skew) for k in ("qweight", "qzeros", "scales")]
    outs = [c.out(k, pc[k], skew=skew) for k in ("qweight", "qzeros", "scales")]
    c.build()
    assert all(b.addr % 16 == skew for b in ins + outs)
    c.run(lambda: _lib().awq_import_gptq(*[b.ptr for b in ins], N, K, gs, 4, int(sym), off, *[b.ptr for b in outs],
                                         _stream(dev)))


# ---------------------------------------------------------------- off the default stream
def test_order_export_import():
    """Both entries, wide and element paths, on a non-blocking stream behind tests/stream_gate.py's
    gate: every launch must be on the caller's stream."""
    from test_stream_order_gpu import walk
    walk([("export_gptq wide", test_export_guard_bands, GUARD[2]),
          ("export_gptq element, ragged qzeros", test_export_guard_bands, GUARD[0]),
          ("export_gptq skewed", test_export_guard_bands, GUARD[3]),
          ("import_gptq wide", test_import_guard_bands, GUARD[2]),
          ("import_gptq element, ragged qzeros", test_import_guard_bands, GUARD[0]),
          ("import_gptq skewed", test_import_guard_bands, GUARD[3])])
