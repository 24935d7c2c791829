"""CPU-only: the host side of include/awq_hip.h's "no global mutable state (re-entrant; one stream
per call)".  awq_last_error is per thread, and the planners (awq_plan_ragged,
awq_plan_block_tensor, awq_stream_plan) called from four threads at once give what they give
serially.  ctypes drops the GIL around every call, so the library's host code does overlap.
(The GPU side: tests/test_stream_order_gpu.py.)"""
import ctypes
import threading

from awq_quantizer import _hip

EINVAL = 1
TIMEOUT = 60.0


def _refused(**kw):
    """awq_quantize_clip_output with NULL pointers: refused before anything is looked at or launched."""
    a = dict(dtype=0, rows=4, K=256, gs=128, bits=4)
    a.update(kw)
    P = ctypes.c_void_p
    return _hip.load_library().awq_quantize_clip_output(P(0), a["dtype"], a["rows"], a["K"], a["gs"], a["bits"], 0, P(0),
                                                        P(0), P(0), 8, a["K"], 20, 0, 10, P(0), P(0), P(0), P(0), P(0),
                                                        P(0), 0, P(0), None)


def test_last_error_is_thread_local():
    """Thread B starts first and reads "" after thread A's refusal; B's own refusal then gives B's
    message, and A still reads its own."""
    _hip.load_library()
    b_started, a_refused, b_refused = threading.Event(), threading.Event(), threading.Event()
    seen = {}

    def thread_b():
        seen["b_first"] = _hip.last_error()
        b_started.set()
        assert a_refused.wait(TIMEOUT)
        seen["b_after_a"] = _hip.last_error()
        seen["b_rc"] = _refused(rows=-1)
        seen["b_own"] = _hip.last_error()
        b_refused.set()

    def thread_a():
        assert b_started.wait(TIMEOUT)
        seen["a_rc"] = _refused(bits=3)
        seen["a_own"] = _hip.last_error()
        a_refused.set()
        assert b_refused.wait(TIMEOUT)
        seen["a_after_b"] = _hip.last_error()

    tb_, ta = threading.Thread(target=thread_b, daemon=True), threading.Thread(target=thread_a, daemon=True)
    tb_.start()
    ta.start()
    ta.join(TIMEOUT)
    tb_.join(TIMEOUT)
    assert not ta.is_alive() and not tb_.is_alive()
    assert seen["a_rc"] == EINVAL and seen["b_rc"] == EINVAL
    assert seen["b_first"] == "" and seen["b_after_a"] == ""
    assert "bit width" in seen["a_own"] and seen["a_after_b"] == seen["a_own"]
    assert "negative" in seen["b_own"] and "bit width" not in seen["b_own"]


# ---------------------------------------------------------------- the planners
RAGGED = [[(3, 1024), (23, 384), (1, 256), (5, 200)],
          [(4096, 128), (1, 128), (7, 2048)],
          [(1, 768)] * 40 + [(768, 768)],
          [(5, 200), (3, 2120), (64, 64), (2, 8192), (9, 136)]]
STREAM = [([(1, 1024), (5, 1024), (1, 1024), (1, 512), (1, 512)], 4096),
          ([(64, 4096)] * 6 + [(1, 128)] * 9, 1 << 20),
          ([(3, 384), (300, 384), (1, 384)], 8192),
          ([(1, 128)] * 50, 4096)]


def plan_ragged(shapes, bits, gs):
    """-> (total tiles, every descriptor's (tile_begin, tile_count), the block table)"""
    lib = _hip.load_library()
    descs = [_hip.TensorDesc(w=16 * (i + 1), rows=r, K=k) for i, (r, k) in enumerate(shapes)]
    total = _hip.plan_ragged(descs, bits, gs)
    arr = (_hip.TensorDesc * len(descs))(*descs)
    n = lib.awq_plan_block_tensor(arr, len(descs), total, None, 0)
    assert n > 0, _hip.last_error()
    table = (ctypes.c_int32 * n)()
    assert lib.awq_plan_block_tensor(arr, len(descs), total, ctypes.cast(table, ctypes.c_void_p), n) == n
    return total, [(d.tile_begin, d.tile_count) for d in descs], list(table)


def plan_stream(shapes, slot):
    lib = _hip.load_library()
    n = len(shapes)
    arr = (_hip.StreamItem * n)()
    for k, (rows, K) in enumerate(shapes):
        arr[k].fd, arr[k].dtype, arr[k].rows, arr[k].K = 0, 0, rows, K
    cfg = _hip.StreamConfig(bits=4, group_size=128, readers=1, nslots=3, slot_bytes=slot, first_batch_bytes=0)
    fb, lb = (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)()
    nb = lib.awq_stream_plan(arr, n, ctypes.byref(cfg), fb, lb)
    assert nb > 0, _hip.last_error()
    return nb, list(fb), list(lb)


def test_planners_from_four_threads():
    """Four threads, each with its own inputs, 200 rounds behind a barrier: every result is the
    serial one."""
    ROUNDS = 200
    work = [((plan_ragged, (RAGGED[t], 4 if t % 2 == 0 else 8, 128)), (plan_stream, STREAM[t])) for t in range(4)]
    serial = [[fn(*args) for fn, args in w] for w in work]
    assert len({repr(s) for s in serial}) == 4                 # different inputs, different plans
    barrier = threading.Barrier(4)
    errors = [None] * 4

    def run(t):
        try:
            barrier.wait(TIMEOUT)
            for r in range(ROUNDS):
                for (fn, args), want in zip(work[t], serial[t]):
                    got = fn(*args)
                    assert got == want, f"thread {t} round {r}: {fn.__name__} differs from the serial plan"
        except BaseException as e:
            errors[t] = e
            barrier.abort()

    threads = [threading.Thread(target=run, args=(t,), daemon=True) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(TIMEOUT)
    assert not any(th.is_alive() for th in threads), "a thread did not finish in time"
    for e in errors:
        if e is not None:
            raise e
