"""Stream ordering for the arena tests: run a call on a fresh non-blocking stream S behind a
device-side gate, so that anything the call puts on another stream is seen.

include/awq_hip.h promises that every launch of an entry point goes to the caller's stream and
that nothing synchronises.  On the legacy default stream, which serialises with everything, a
launch on the wrong stream computes the right bytes all the same.  Inside `with ordered(dev):`
  * torch's current stream is S, so every `_stream(dev)` of the tests and every wrapper of
    awq_quantizer/_hip.py resolves to S;
  * Call.run (tests/test_gpu_bounds.py) and run_tensors() below make the call's memory *stale*
    (the bitwise complement of what the call must see), synchronise, and then put on S, in order:
    the gate (a device-side spin of GATE_MS), the restore of the real contents, the call;
  * while the gate still spins they synchronise stream 0 — S is non-blocking, so this returns at
    once unless the call put something there, and that something has then run on stale memory:
    a misplaced reader saw the complement of its inputs, a misplaced writer (kernel or memset) is
    overwritten by the restore, a misplaced later stage read a workspace that held the fill;
  * `gate_done.query()` must still be False after that synchronise.  That assertion, not the
    duration, is what makes a pass a proof: if it fails the case raises GateUnproven (a setup
    error naming the case), never a pass.

Pointer-bearing inputs (the ragged launch's descriptors and block table) keep their real contents
while the rest is stale: a misplaced kernel may only ever compute wrong numbers, never form an
address from junk.  Everything else the enrolled kernels read is arithmetic only — packed words,
scales, tables, statistics — and every extent comes from by-value arguments.

Two things keep a gate from proving nothing.  The runtime loads a kernel's code at its first launch
(tens of milliseconds of host time), so every call is launched once, untimed, before its memory
goes stale.  And the runtime maps streams onto a few hardware queues: a fresh stream that shares
stream 0's queue would make stream 0 wait for the gate, so independent_stream() tries candidates
with the precondition itself and takes the first that stream 0 does not wait for.

The gate is torch.cuda._sleep(cycles), calibrated once per session against torch.cuda.Event.
GATE_MS is ten times the longest host span (gate issued .. stream 0 synchronised) measured over
the enrolled cases on an MI355X; it is a detection window, not a performance figure."""
import contextlib
import gc
import time

import torch

MEASURED_SPAN_MS = 0.15   # the longest span of any enrolled case on an MI355X (0.148 ms)
GATE_MS = 10 * MEASURED_SPAN_MS

_active = None
_cycles_per_ms = {}


class GateUnproven(RuntimeError):
    """The gate had ended before stream 0 was synchronised: the case proved nothing."""


def active():
    """The Ordered context in force, or None (Call.run then behaves as it always has)."""
    return _active


def cycles_per_ms(dev) -> float:
    """Calibrate torch.cuda._sleep against event timing, once per session and device."""
    key = torch.device(dev).index or 0
    if key not in _cycles_per_ms:
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            torch.cuda._sleep(1_000_000)                      # load the kernel
            best = 0.0
            for cycles in (20_000_000, 20_000_000):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                torch.cuda._sleep(cycles)
                b.record(s)
                s.synchronize()
                best = max(best, cycles / a.elapsed_time(b))  # the shorter time: less launch overhead in it
        _cycles_per_ms[key] = best
    return _cycles_per_ms[key]


STREAM_TRIES = 8


def independent_stream(dev, cycles):
    """-> (a fresh stream that stream 0 does not queue behind, the streams tried before it).
    The runtime maps streams onto a few hardware queues (4 by default), so one fresh stream in
    four shares stream 0's queue: a kernel on stream 0 would then wait for the gate, and a
    misplaced launch would show as an unproven gate instead of wrong bytes.  Each candidate is
    tried with the precondition itself: the gate on it, one op on stream 0, stream 0 synchronised,
    the gate still running."""
    zero = torch.cuda.default_stream(dev)
    with torch.cuda.stream(zero):
        probe = torch.zeros(64, device=dev)
        probe.add_(1)                                   # (loaded before it is timed)
    torch.cuda.synchronize(dev)
    for tried in range(STREAM_TRIES):
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            done = torch.cuda.Event()
            done.record(s)
        with torch.cuda.stream(zero):
            probe.add_(1)
        zero.synchronize()
        free = not done.query()
        s.synchronize()
        if free:
            return s, tried
    raise GateUnproven(f"stream 0 waited for the gate on each of {STREAM_TRIES} fresh streams: on this runtime no case can "
                       f"prove anything")


class Ordered:
    def __init__(self, dev, gate_ms):
        self.dev, self.gate_ms = dev, gate_ms
        self.cycles = int(gate_ms * cycles_per_ms(dev))
        self.stream, self.streams_skipped = independent_stream(dev, self.cycles)
        self.case = "?"             # set by the walker, named by every error
        self.spans = []             # (seconds from the gate's issue to the end of step 4, case); non-blocking calls
        self.gates = 0

    def gate(self) -> torch.cuda.Event:
        """Put the gate on S; -> the event recorded right behind it."""
        torch.cuda._sleep(self.cycles)
        done = torch.cuda.Event()
        done.record(self.stream)
        self.gates += 1
        return done

    def behind_gate(self, restore, call, *, blocks=False):
        """Steps 3 to 5: on S the gate, restore(), call(); stream 0 synchronised while the gate
        spins; S synchronised.  blocks: the call itself waits for S on the host (its result is a
        host value), so step 4 cannot hold and only the result's equality is left to assert."""
        assert torch.cuda.current_stream(self.dev) == self.stream
        collecting = gc.isenabled()
        gc.disable()                # (a collection is host time the gate would have to outlast)
        try:
            t0 = time.perf_counter()
            done = self.gate()
            restore()
            result = call()
            torch.cuda.default_stream(self.dev).synchronize()
            early = done.query()
        finally:
            if collecting:
                gc.enable()
        if not blocks:
            self.spans.append((time.perf_counter() - t0, self.case))
        self.stream.synchronize()
        if early and not blocks:
            raise GateUnproven(f"{self.case}: the gate of {self.gate_ms} ms had ended when stream 0 was synchronised "
                               f"({(time.perf_counter() - t0) * 1e3:.2f} ms after its issue, S's synchronise included): nothing is proven")
        return result

    def longest_span_ms(self):
        return max(((s * 1e3, c) for s, c in self.spans), default=(0.0, None))


@contextlib.contextmanager
def ordered(dev, gate_ms=None):
    """Enter torch.cuda.stream(S) for a fresh S and switch Call.run / run_tensors to ordered mode."""
    global _active
    assert _active is None, "ordered() does not nest"
    st = Ordered(dev, GATE_MS if gate_ms is None else gate_ms)
    torch.cuda.synchronize(dev)
    _active = st
    try:
        with torch.cuda.stream(st.stream):
            w = torch.zeros(4096, dtype=torch.uint8, device=dev)    # the protocol's own torch kernels, loaded
            torch.bitwise_not(w.clone(), out=w)                     # before any gate (a first launch costs
            w.copy_(w.clone())                                      # tens of milliseconds)
            torch.cuda._sleep(1000)
            st.stream.synchronize()
            yield st
    finally:
        _active = None
        torch.cuda.synchronize(dev)


def _u8(t):
    return t.detach().reshape(-1).view(torch.uint8)


def stale(tensors):
    """-> shadows; every (contiguous) tensor then holds the complement of its bytes."""
    shadows = [t.clone() for t in tensors]
    for t in tensors:
        u = _u8(t)
        u.copy_(~u)
    return shadows


def run_tensors(st: Ordered, tensors, call, *, pointers=(), blocks=False):
    """The protocol without an arena, for the wrappers: `tensors` are the device tensors the call
    reads (accumulators it adds to included; all contiguous); `pointers` are read too but hold
    addresses or indices and stay real."""
    for t in list(tensors) + list(pointers):
        assert t.is_cuda and t.is_contiguous()
    shadows = stale(tensors)
    torch.cuda.synchronize(st.dev)

    def restore():
        for t, s in zip(tensors, shadows):
            t.copy_(s)
    return st.behind_gate(restore, call, blocks=blocks)
