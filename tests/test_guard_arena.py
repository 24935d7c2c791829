"""The guard-band arena itself (tests/guard_arena.py): placement arithmetic, and proof that a
one-byte write outside a view — or inside an input marked untouched — is caught and reported with
the buffer's name, the side and the offset, on the CPU and (one gpu-marked copy) on the device."""
import pytest
import torch

from guard_arena import GUARD, Arena, GuardError


def _arena(device="cpu"):
    a = Arena(Arena.required([1000, 6, 64, 4096]), device)
    regs = [a.place(1000, name="first"), a.place(6, align=16, skew=2, name="skewed"),
            a.place(64, align=256, skew=4, name="third"), a.place(4096, align=4096, name="page")]
    return a, regs


def test_skew_and_alignment_arithmetic():
    a, (r0, r1, r2, r3) = _arena()
    assert a.buf.data_ptr() % 4096 == 0
    assert r0.data_ptr() % 256 == 0 and r0.nbytes == 1000 and r0.u8.numel() == 1000
    assert r1.data_ptr() % 16 == 2 and r1.nbytes == 6
    assert r2.data_ptr() % 256 == 4
    assert r3.data_ptr() % 4096 == 0
    for r in (r0, r1, r2, r3):
        assert r.u8.data_ptr() == r.data_ptr()
    assert r1.view(torch.bfloat16, (3,)).shape == (3,) and r1.view(torch.bfloat16).data_ptr() == r1.data_ptr()
    assert r2.view(torch.float32, (4, 4)).shape == (4, 4)
    with pytest.raises(ValueError):
        r1.view(torch.float32)                      # 2-B residue, 4-B elements
    with pytest.raises(ValueError):
        r2.view(torch.float32, (3, 4))              # not the whole view
    with pytest.raises(ValueError):
        a.place(8, align=16, skew=16)
    with pytest.raises(ValueError):
        Arena(GUARD, "cpu").place(1)                # no room for the second guard


def test_neighbouring_placement():
    """Views come in call order; between two neighbours lies one guard band, widened only by the
    padding the second view's residue needs; a band lies before the first and after the last."""
    a, regs = _arena()
    assert regs[0].start >= GUARD
    for p, n in zip(regs, regs[1:]):
        assert p.end + GUARD <= n.start < p.end + GUARD + 4096
    assert a.capacity - regs[-1].end >= GUARD
    b = Arena(Arena.required([512, 512]), "cpu")
    x, y = b.place(512), b.place(512)
    assert y.start - x.end == GUARD                 # both 256-aligned: the band alone


def test_fill_is_position_dependent_and_complemented():
    a, regs = _arena()
    a.fill(3)
    one = a.buf.clone()
    a.check()
    assert len(torch.unique(one[:4096])) > 200      # no constant sentinel
    assert not torch.equal(one[:GUARD], one[GUARD:2 * GUARD])
    a.fill(3, complement=True)
    assert torch.equal(a.buf, ~one)
    a.fill(4)
    assert not torch.equal(a.buf, one)
    assert torch.equal(a.fill_of(regs[1]), a.buf[regs[1].start:regs[1].end])
    with pytest.raises(RuntimeError):
        a.place(8)                                  # the fill would not cover its guards


def _one_byte_before_and_after(device):
    a, regs = _arena(device)
    a.fill(11)
    a.check()
    for r in regs:                                  # writes inside the views are the test's own business
        r.u8[:] = 0x5A
    a.check()
    tgt = regs[2]
    a.buf[tgt.start - 1] = a.buf[tgt.start - 1] ^ 0x01
    with pytest.raises(GuardError) as e:
        a.check()
    assert "before the start of 'third'" in str(e.value) and "offsets -1 .. -1" in str(e.value)
    assert "1 byte(s)" in str(e.value) and "skewed" not in str(e.value)
    a.fill(11)
    a.buf[tgt.end] = a.buf[tgt.end] ^ 0x80
    with pytest.raises(GuardError) as e:
        a.check()
    assert "after the end of 'third'" in str(e.value) and "offsets +0 .. +0" in str(e.value)
    assert "page" not in str(e.value)
    a.fill(11)
    a.buf[tgt.end + 5:tgt.end + 9] = a.buf[tgt.end + 5:tgt.end + 9] ^ 0xFF
    a.buf[a.capacity - 1] = a.buf[a.capacity - 1] ^ 0xFF
    with pytest.raises(GuardError) as e:
        a.check()
    assert "after the end of 'third': 4 byte(s) changed, offsets +5 .. +8" in str(e.value)
    assert "after the end of 'page': 1 byte(s)" in str(e.value)


def test_one_byte_before_and_after_a_view_is_caught():
    _one_byte_before_and_after("cpu")


@pytest.mark.gpu
def test_one_byte_before_and_after_a_view_is_caught_on_the_device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _one_byte_before_and_after(torch.device("cuda", 0))


def test_complement_run_catches_a_byte_equal_to_the_fill():
    """A stray write of a value that happens to equal the fill passes in one polarity and is
    caught in the other."""
    a, regs = _arena()
    a.fill(5)
    pos = regs[0].end + 3
    value = int(a.buf[pos])
    a.buf[pos] = value                              # the "overrun" writes what is already there
    a.check()
    a.fill(5, complement=True)
    a.buf[pos] = value
    with pytest.raises(GuardError) as e:
        a.check()
    assert "after the end of 'first'" in str(e.value) and "offsets +3 .. +3" in str(e.value)


def test_untouched_view_catches_an_in_place_write():
    a = Arena(Arena.required([256, 256]), "cpu")
    w = a.place(256, name="w", untouched=True)
    out = a.place(256, name="out")
    a.fill(9)
    x = torch.arange(64, dtype=torch.float32)
    w.store(x)
    out.view(torch.float32)[:] = w.view(torch.float32) * 2
    a.check()
    w.view(torch.float32)[17] *= 2                  # an in-place write into the input
    with pytest.raises(GuardError) as e:
        a.check()
    assert "inside 'w' (must stay untouched)" in str(e.value) and "offsets +70 .. +71" in str(e.value)
    a.mark_untouched(w, False)
    a.check()
