"""Guard-band arena for the bounds tests (tests/test_gpu_bounds.py): one uint8 tensor, on the CPU
or the GPU, out of which a test places every input, output and workspace of a call.

  * place() hands out views of exactly the size asked for, at a chosen address residue, in call
    order; a guard band of GUARD bytes lies directly before every view and directly after its last
    byte (two neighbours share the band between them, widened only by alignment padding);
  * fill() writes a position-dependent pseudo-random byte stream — or its bitwise complement — over
    the whole arena, views included: an output byte a kernel skips holds the fill, which is wrong
    in at least one of the two polarities, and an over-read sees different data in the two;
  * check() compares every byte outside the placed views (and inside the views marked
    "untouched") with the fill, and raises GuardError naming the buffer, the side and the first
    and last offset touched.

GUARD is 64 KiB: eight times the largest footprint one wave stores (2048 elements x 4 B of
tensor_q).  It is a detection window, not a measurement."""
from __future__ import annotations

import torch

GUARD = 64 * 1024
_BASE_ALIGN = 4096
_CHUNK = 1 << 20


class GuardError(AssertionError):
    """A byte outside the placed views (or inside an untouched one) no longer holds the fill."""


class Region:
    """One placed view: bytes [start, end) of the arena."""

    def __init__(self, arena, name, start, nbytes, untouched):
        self.arena, self.name, self.start, self.end, self.untouched = arena, name, start, start + nbytes, untouched

    @property
    def nbytes(self) -> int:
        return self.end - self.start

    @property
    def u8(self) -> torch.Tensor:
        return self.arena.buf[self.start:self.end]

    def view(self, dtype: torch.dtype, shape=None) -> torch.Tensor:
        """The region as a typed tensor (its whole size unless a shape is given; the shape must
        fill the region exactly)."""
        size = torch.empty((), dtype=dtype).element_size()
        if self.data_ptr() % size or self.nbytes % size:
            raise ValueError(f"{self.name}: address or size is not a multiple of the {size}-byte element")
        t = self.u8.view(dtype)
        if shape is not None:
            n = 1
            for d in shape:
                n *= int(d)
            if n * size != self.nbytes:
                raise ValueError(f"{self.name}: shape {tuple(shape)} of {dtype} is not {self.nbytes} bytes")
            t = t.reshape(shape)
        return t

    def data_ptr(self) -> int:
        return self.arena.buf.data_ptr() + self.start

    def store(self, t: torch.Tensor) -> None:
        """Copy a (CPU or device) tensor's bytes into the view; sizes must match exactly."""
        src = t.detach().contiguous().reshape(-1).view(torch.uint8)
        if src.numel() != self.nbytes:
            raise ValueError(f"{self.name}: {src.numel()} bytes stored into a view of {self.nbytes}")
        self.u8.copy_(src)
        if self.arena._fill is not None:            # an untouched view must keep what was stored
            self.arena._fill[self.start:self.end] = self.u8

    def load(self, dtype: torch.dtype, shape=None) -> torch.Tensor:
        """The view's bytes as a CPU tensor of dtype (a copy; any address residue)."""
        t = self.u8.cpu().clone().view(dtype)
        return t if shape is None else t.reshape(shape)


class Arena:
    def __init__(self, capacity: int, device="cpu"):
        """capacity: bytes available to place() (views, guards and alignment padding)."""
        self.device = torch.device(device)
        raw = torch.empty(capacity + _BASE_ALIGN, dtype=torch.uint8, device=self.device)
        off = (-raw.data_ptr()) % _BASE_ALIGN
        self._raw = raw
        self.buf = raw[off:off + capacity]          # base address a multiple of 4096
        self.capacity = capacity
        self.regions = []
        self._fill = None
        self._cursor = 0                            # end of the last view

    @staticmethod
    def required(sizes, align: int = 4096) -> int:
        """A capacity that holds views of these sizes, each at any residue of up to `align`."""
        return sum(GUARD + align + int(n) for n in sizes) + GUARD

    # ------------------------------------------------------------------ placement
    def place(self, nbytes: int, align: int = 256, skew: int = 0, name: str = None, untouched: bool = False) -> Region:
        """A view of exactly nbytes whose address is = skew (mod align), GUARD bytes after the
        previous view's end (plus the padding the residue needs)."""
        if nbytes < 0 or align <= 0 or not 0 <= skew < align:
            raise ValueError("place: nbytes >= 0, align > 0, 0 <= skew < align")
        if self._fill is not None:
            raise RuntimeError("place after fill: the fill would not cover the new view's guards")
        base = self.buf.data_ptr()
        start = self._cursor + GUARD
        start += (skew - (base + start)) % align
        if start + nbytes + GUARD > self.capacity:
            raise ValueError(f"arena of {self.capacity} bytes is full (need {start + nbytes + GUARD})")
        r = Region(self, name or f"buffer{len(self.regions)}", start, nbytes, untouched)
        self.regions.append(r)
        self._cursor = start + nbytes
        return r

    def mark_untouched(self, region: Region, flag: bool = True) -> None:
        region.untouched = flag

    # ------------------------------------------------------------------ fill
    def _stream(self, seed: int, lo: int, hi: int) -> torch.Tensor:
        """Bytes [lo, hi) of the fill stream of `seed`: a function of the offset in the arena and
        the seed alone (31-bit integer mixing carried in int64, so no product overflows)."""
        i = torch.arange(lo, hi, dtype=torch.int64, device=self.device)
        m = 0x7FFFFFFF
        h = (i * 1103515245 + (12345 + 7919 * (seed & 0xFFFF))) & m
        h = ((h ^ (h >> 15)) * 0x2C1B3C6D) & m
        h = ((h ^ (h >> 12)) * 0x297A2D39) & m
        h = h ^ (h >> 15)
        return (h & 0xFF).to(torch.uint8)

    def fill(self, seed: int, complement: bool = False) -> None:
        """Overwrite the whole arena — guards, views and gaps — with the seed's byte stream, or
        with its bitwise complement."""
        if self._fill is None:
            self._fill = torch.empty_like(self.buf)
        for lo in range(0, self.capacity, _CHUNK):
            hi = min(lo + _CHUNK, self.capacity)
            s = self._stream(seed, lo, hi)
            self._fill[lo:hi] = ~s if complement else s
        self.buf.copy_(self._fill)

    def fill_of(self, region: Region) -> torch.Tensor:
        """What fill() wrote into a region (CPU uint8 copy)."""
        return self._fill[region.start:region.end].cpu()

    # ------------------------------------------------------------------ check
    def check(self) -> None:
        if self._fill is None:
            raise RuntimeError("check before fill")
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        bad = self.buf != self._fill
        for r in self.regions:
            if not r.untouched:
                bad[r.start:r.end] = False
        if not bool(bad.any()):
            return
        idx = torch.nonzero(bad).reshape(-1).cpu()
        msgs = []

        def report(lo, hi, what, ref, sign):
            sel = idx[(idx >= lo) & (idx < hi)]
            if sel.numel():
                a, b = int(sel.min()) - ref, int(sel.max()) - ref
                msgs.append(f"{what}: {sel.numel()} byte(s) changed, offsets {a:+d} .. {b:+d} relative to {sign}")

        prev_end, prev = 0, None
        for r in self.regions:
            # the gap before r: its first half belongs to the previous view's end, the rest to r's start
            mid = prev_end + (r.start - prev_end) // 2 if prev is not None else 0
            if prev is not None:
                report(prev_end, mid, f"after the end of '{prev.name}'", prev_end, "one past its last byte")
            report(mid, r.start, f"before the start of '{r.name}'", r.start, "its first byte")
            if r.untouched:
                report(r.start, r.end, f"inside '{r.name}' (must stay untouched)", r.start, "its first byte")
            prev_end, prev = r.end, r
        if prev is not None:
            report(prev_end, self.capacity, f"after the end of '{prev.name}'", prev_end, "one past its last byte")
        else:
            report(0, self.capacity, "in an arena without views", 0, "the arena's first byte")
        raise GuardError("; ".join(msgs))
