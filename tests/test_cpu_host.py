"""CPU-only tests: the C-ABI library loads and exports every declared symbol, and the
drop-in host layer keeps the reference's interface (validation, defaults, errors,
skip semantics) — no kernel is launched here."""
import ctypes
import os
import re

import pytest
import torch

import golden_io as gio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    """Every entry point declared by include/*.h (awq_hip.h, awq_ptfile.h)."""
    src = ""
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h.endswith(".h"):
            with open(os.path.join(ROOT, "include", h)) as f:
                src += f.read()
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|uint32_t|const char\*)\s+(awq_\w+)\s*\(", src, re.M)))


def test_library_exports_every_declared_symbol():
    from awq_quantizer import _hip
    lib = _hip.load_library()
    syms = declared_symbols()
    assert len(syms) >= 10
    for s in syms:
        assert hasattr(lib, s), s
    assert set(syms) == set(_hip.SIGNATURES), "python binding out of sync with include/*.h"
    assert lib.awq_abi_version() == _hip.ABI_VERSION == 17


def test_product_library_has_no_diagnostics_entry_points():
    """one path per shape in the shipped library — no tuning entry point
    (it lives in the diagnostics build only, with the A/B kernel variants)."""
    from awq_quantizer import _hip
    lib = _hip.load_library()
    assert not hasattr(lib, "awq_set_tuning")
    if os.path.exists(_hip.DIAG_LIB_PATH):
        assert hasattr(_hip.load_diag_library(), "awq_set_tuning")
    for mod in ("main", "options", "output", "pipeline", "fold_cli", "dist_cli"):     # the CLI's modules
        src = open(os.path.join(ROOT, "awq-converter_amd", "awq_quantizer", mod + ".py")).read()
        assert "os.environ" not in src.replace('os.environ.get("AWQ_DIST_BACKEND"', ""), mod


def test_diag_tuning_rejects_a_retired_fp64_span():
    """gen_noreg selects the fp64 span: 0 the LDS span, 1 the strided one; the register span (2) is
    gone, and awq_set_tuning says so instead of silently taking the default."""
    from awq_quantizer import _hip
    diag = _hip.load_diag_library()
    for v, rc in ((0, 0), (1, 0), (2, -1), (-1, -1)):
        t = _hip.Tuning(gen_noreg=v)
        assert (diag.awq_set_tuning(ctypes.byref(t)) == 0) == (rc == 0), v
    assert diag.awq_set_tuning(None) == 0
    assert not hasattr(_hip.Tuning(), "dq_words_v1")
    assert ctypes.sizeof(_hip.Tuning) == 11 * 4


def test_library_is_gfx950_code_object():
    from awq_quantizer import _hip
    data = open(_hip.LIB_PATH, "rb").read()
    assert b"gfx950" in data


def test_host_helpers_without_gpu():
    from awq_quantizer import _hip
    lib = _hip.load_library()
    assert lib.awq_ragged_eligible(0, 1024, 4096, 128) == 1
    assert lib.awq_ragged_eligible(0, 1024, 4000, 128) == 1     # padded rows: 4000 % 8 == 0
    assert lib.awq_ragged_eligible(0, 1024, 4001, 128) == 0
    assert lib.awq_ragged_eligible(1, 1024, 4096, 128) == 1     # fp16 streams too
    assert lib.awq_ragged_eligible(2, 1024, 4096, 128) == 1     # fp32 streams too
    assert lib.awq_ragged_eligible(3, 1024, 4096, 128) == 0     # fp64 -> generic kernel
    d = [_hip.TensorDesc(4096 * 16, 1024, 4096, 0, 0, 2 * 4096, 0, 0, 0, 0),
         _hip.TensorDesc(4096 * 32, 1, 768, 0, 0, 2 * 8192, 0, 0, 0, 0),
         _hip.TensorDesc(4096 * 48, 50, 768, 0, 0, 2 * 16384, 0, 0, 0, 0)]
    total = _hip.plan_ragged(d, 4)
    # 1024 rows x G=32 -> 16-group tiles -> 2048; G=6 (even) -> byte tiles: 16 flat groups
    assert d[0].tile_count == 2048 and d[1].tile_count == 1 and d[2].tile_count == 19
    assert total == 2048 + 1 + 19 and d[2].tile_begin == 2049
    # tensor table: entry b (64 B = 16 int32) covers the 8 tiles t0, t0 + 8, ..., t0 + 56 of
    # one XCD (tile t runs on XCD t % 8) inside a 64-tile window, the two windows of a
    # 128-tile pair side by side (index (t >> 7) * 16 + (t & 7) * 2 + ((t >> 6) & 1)): the
    # tensor's input pointer, first tile, rows, K, then its index (bit 31: the entry spans)
    arr = (_hip.TensorDesc * 3)(*d)
    n_ent = -(-total // 128) * 16
    assert lib.awq_plan_block_tensor(arr, 3, total, None, 0) == n_ent * 16
    tab = torch.full(((n_ent + 20) * 16,), -7, dtype=torch.int32)
    assert lib.awq_plan_block_tensor(arr, 3, total, ctypes.c_void_p(tab.data_ptr()), (n_ent + 20) * 16) == n_ent * 16
    e = tab[:n_ent * 16].view(n_ent, 16)
    q = e.view(torch.int64)                      # [n, 8]: w, tile_begin, rows, K, ...
    begins = [arr[i].tile_begin for i in range(3)]

    def owner(t):
        return max(i for i in range(3) if begins[i] <= t)
    for b in range(n_ent):
        t0 = min((b >> 4) * 128 + (b & 1) * 64 + ((b & 15) >> 1), total - 1)
        last = max(t0, min(t0 + 56, total - 1))
        cur = owner(t0)
        spans = owner(last) != cur
        assert e[b, 8].item() == (cur | (-2**31 if spans else 0)), b
        assert q[b, 0].item() == d[cur].w and q[b, 1].item() == begins[cur]
        assert q[b, 2].item() == d[cur].rows and q[b, 3].item() == d[cur].K
    for t in range(total):                       # every tile's entry starts at or before it
        b = (t >> 7) * 16 + (t & 7) * 2 + ((t >> 6) & 1)
        first = (b >> 4) * 128 + (b & 1) * 64 + ((b & 15) >> 1)
        assert first <= t and (t - first) % 8 == 0 and t - first <= 56
    assert tab[n_ent * 16:].eq(-7).all()
    assert lib.awq_plan_block_tensor(arr, 3, total, ctypes.c_void_p(tab.data_ptr()), 100) < 0
    # G odd at 4 bits -> word tiles: K=384 (G=3) -> 5 rows (15 groups) per tile
    d = [_hip.TensorDesc(4096 * 16, 11, 384, 0, 0, 2 * 4096, 0, 0, 0, 0)]
    assert _hip.plan_ragged(d, 4) == 3
    d = [_hip.TensorDesc(4096 * 16, 11, 384, 0, 0, 2 * 4096, 0, 0, 0, 0)]
    assert _hip.plan_ragged(d, 8) == 3   # 8-bit: byte tiles, 33 groups -> 3
    # other group sizes: a tile is 2048 elements = 2048 / gs group slots
    for gs in (32, 64, 128, 256):
        assert lib.awq_ragged_eligible(0, 1024, 4096, gs) == 1
        assert lib.awq_ragged_eligible(1, 7, 3 * gs, gs) == 1
        assert lib.awq_ragged_eligible(0, 7, 3 * gs + 8, gs) == 1   # padded rows (K % 8 == 0) stream too
        assert lib.awq_ragged_eligible(0, 7, 3 * gs + 4, gs) == 0   # K % 8 != 0 -> generic
    for gs in (16, 100, 512):
        assert lib.awq_ragged_eligible(0, 1024, 4096, gs) == 0
    d = [_hip.TensorDesc(4096 * 16, 1024, 4096, 0, 0, 2 * 4096, 0, 0, 0, 0)]
    assert _hip.plan_ragged(d, 4, 32) == 1024 * 4096 // 2048        # byte tiles, 64 groups each
    d = [_hip.TensorDesc(4096 * 16, 11, 96, 0, 0, 2 * 4096, 0, 0, 0, 0)]
    assert _hip.plan_ragged(d, 4, 32) == 1   # G=3 odd -> word tiles of 21 whole rows (63 groups)
    d = [_hip.TensorDesc(4096 * 16, 11, 768, 0, 0, 2 * 4096, 0, 0, 0, 0)]
    assert _hip.plan_ragged(d, 4, 256) == 6   # gs 256: 8 slots; G=3 odd, WPR=1 -> 2 whole rows per tile
    d = [_hip.TensorDesc(4096 * 16, 11, 768, 0, 0, 2 * 4096, 0, 0, 0, 0)]
    assert _hip.plan_ragged(d, 8, 256) == 5   # 8-bit: byte tiles, 33 groups / 8 -> 5
    with pytest.raises(RuntimeError, match="group_size"):
        _hip.plan_ragged(d, 4, 100)
    # padded rows: row tiles, ceil(G / S) per row (K = 4544, gs 128: G = 36 -> 3 tiles per row)
    d = [_hip.TensorDesc(4096 * 16, 11, 4544, 0, 0, 2 * 4096, 0, 0, 0, 0)]
    assert _hip.plan_ragged(d, 4, 128) == 33
    assert _hip.ragged_flags(d, 128) == 1 and _hip.ragged_flags(d, 64) == 0   # 4544 = 71 x 64
    d = [_hip.TensorDesc(4096 * 16, 1, 5000, 0, 0, 2 * 4096, 0, 0, 0, 0)]
    assert _hip.plan_ragged(d, 4, 256) == 3          # G = 20, 8 slots per tile
    # validation errors come back with a message, nothing launched
    assert lib.awq_quantize_groups(None, 0, 4, 256, 128, 3, 0, None, None, None, None, None, None) != 0
    assert "bit width" in _hip.last_error()
    assert lib.awq_quantize_groups(None, 0, 4, 256, 0, 4, 0, None, None, None, None, None, None) != 0
    assert "Group size" in _hip.last_error()


@pytest.mark.parametrize("rec", gio.manifest()["validation"], ids=lambda r: str(r.get("params", r.get("quantize_arg"))))
def test_validation_matches_reference(rec):
    from awq_quantizer.quantization import AWQQuantizer
    if "params" in rec:
        with pytest.raises(ValueError) as e:
            AWQQuantizer(device="cpu", logger_level="ERROR", **rec["params"])
        assert str(e.value) == rec["message"]
    else:
        q = AWQQuantizer(device="cpu", logger_level="ERROR")
        arg = [1.0, 2.0] if rec["quantize_arg"] == "list" else torch.arange(256, dtype=torch.int32)
        with pytest.raises(ValueError) as e:
            q.quantize(arg)
        assert str(e.value) == rec["message"]


def test_defaults_and_ranges():
    from awq_quantizer.quantization import AWQQuantizer
    q = AWQQuantizer(logger_level="ERROR")
    assert (q.bits, q.group_size, q.symmetric, q.zero_point, q.scale_method, q.per_channel) == \
        (4, 128, True, "minmax", "mse", True)
    assert (q.qmin, q.qmax) == (-8, 7)
    assert AWQQuantizer(symmetric=False, logger_level="ERROR")._calculate_qmin_qmax() == (0, 15)
    assert AWQQuantizer(bits=8, symmetric=False, logger_level="ERROR")._calculate_qmin_qmax() == (0, 255)
    assert AWQQuantizer(bits=8, logger_level="ERROR")._calculate_qmin_qmax() == (-128, 127)
    if not torch.cuda.is_available():
        assert q.device == "cpu"
        assert AWQQuantizer(device="cuda:3", logger_level="ERROR").device == "cpu"


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback():
    from awq_quantizer import _hip
    from awq_quantizer.quantization import AWQQuantizer
    q = AWQQuantizer(device="cpu", logger_level="ERROR")
    with pytest.raises(_hip.HipUnavailable):
        q.quantize(torch.randn(4, 256, dtype=torch.bfloat16))
    # quantize_model keeps the reference's skip-and-log behaviour: nothing quantized
    assert q.quantize_model({"a": torch.randn(4, 256, dtype=torch.bfloat16)}) == {}


def test_small_and_empty_errors_before_device():
    from awq_quantizer.quantization import AWQQuantizer
    q = AWQQuantizer(device="cpu", logger_level="ERROR")
    with pytest.raises(RuntimeError):
        q.quantize(torch.zeros(0, dtype=torch.bfloat16))
    with pytest.raises(TypeError):
        AWQQuantizer(device="cpu", zero_point="percentile", logger_level="ERROR").quantize(
            torch.randn(4, 256, dtype=torch.bfloat16))


def test_packed_shapes():
    from awq_quantizer.quantization import AWQQuantizer
    q = AWQQuantizer(bits=4, logger_level="ERROR")
    sh = q.packed_shapes((4096, 14336))
    assert sh["qweight"] == (4096, 1792) and sh["qzeros"] == (4096, 14) and sh["scales"] == (4096, 112)
    sh = AWQQuantizer(bits=8, logger_level="ERROR").packed_shapes((768,))
    assert sh["qweight"] == (1, 192) and sh["qzeros"] == (1, 2) and sh["scales"] == (1, 6)


def test_bench_valu_roofline_issue_slot_model(tmp_path):
    """bench.py's VALU roofline: peak = 614.4 G issue slots/s / the kernel's recorded slots per
    unit ((SQ_ACTIVE_INST_VALU - SQ_ACTIVE_INST_VALU2) / units); records made on other kernel
    sources or without the dual-issue counter are not used."""
    import json
    import sys
    sys.path.insert(0, ROOT)
    import bench
    assert bench.VALU_SLOT_RATE == 256 * 4 * 2.4e9 / 4
    now = bench.kernel_source_hash(bench.KERNEL_SOURCES)
    p = tmp_path / "valu.json"
    p.write_text(json.dumps({
        "ok": {"valu_slots_per_unit": 0.25, "kernel_source_sha256": now},
        "stale": {"valu_slots_per_unit": 0.25, "kernel_source_sha256": "0" * 16},
        "old": {"valu_lane_instr_per_unit": 14.5, "kernel_source_sha256": now}}))
    per, src = bench.recorded_valu(str(p), "ok", bench.KERNEL_SOURCES)
    assert per == 0.25 and src["stale"] is False
    r = bench.valu_roofline(1e12, 1.0, per, src, "candidate-elements")
    assert r["peak"] == round(bench.VALU_SLOT_RATE / 0.25 / 1e9, 2)
    assert r["frac"] == round(1000.0 / (bench.VALU_SLOT_RATE / 0.25 / 1e9), 4)
    assert bench.recorded_valu(str(p), "stale", bench.KERNEL_SOURCES)[0] is None
    assert bench.recorded_valu(str(p), "old", bench.KERNEL_SOURCES)[0] is None
    assert bench.recorded_valu(str(p), "missing", bench.KERNEL_SOURCES) == (None, None)


def test_abi17_argument_validation_without_gpu():
    """The round-6 entry points reject bad arguments before anything is launched: integer op
    dtypes only in dequantize mode, no uint16/32/64 / bool op dtypes, _UNSIGNED only with _INT,
    unknown flags; awq_group_params_ex flags; awq_dequant_ceiling sizes and alignment."""
    from awq_quantizer import _hip
    lib = _hip.load_library()
    P = ctypes.c_void_p(64)
    null = None
    # x int64 (5) quantized with int64 op dtypes: mode 0 divides -> float ops only
    assert lib.awq_apply_params_ex(P, 5, 1, 8, 8, P, P, 0, 15, 0, 5, 5, 0, P, null) != 0
    assert "floating point" in _hip.last_error()
    for bad_op in (9, 10, 11, 12, 13, -1):            # bool / uint16 / uint32 / uint64 / unknown
        assert lib.awq_apply_params_ex(P, 5, 1, 8, 8, P, P, 0, 15, 1, bad_op, 2, 0, P, null) != 0
        assert "op dtype" in _hip.last_error()
    assert lib.awq_apply_params_ex(P, 13, 1, 8, 8, P, P, 0, 15, 1, 2, 2, 0, P, null) != 0   # x dtype 13
    assert lib.awq_apply_params_ex(P, 5, 1, 8, 8, P, P, 0, 15, 1, 5, 5, _hip.APPLY_SCALE_UNSIGNED, P, null) != 0
    assert "_INT" in _hip.last_error()
    assert lib.awq_apply_params_ex(P, 5, 1, 8, 8, P, P, 0, 15, 1, 5, 5, 128, P, null) != 0
    assert "unknown flags" in _hip.last_error()
    # every valid combination of sizes 0 returns before touching a pointer or the device
    allf = (_hip.APPLY_SCALE_ONE_ELEMENT | _hip.APPLY_ZERO_ONE_ELEMENT | _hip.APPLY_SCALE_INT | _hip.APPLY_ZERO_INT
            | _hip.APPLY_SCALE_UNSIGNED | _hip.APPLY_ZERO_UNSIGNED | _hip.APPLY_IEEE_CLAMP)
    assert lib.awq_apply_params_ex(null, 12, 0, 8, 8, null, null, 0, 15, 0, 2, 2, allf, null, null) == 0
    assert lib.awq_group_params_ex(P, 0, 1, 128, 128, 4, 0, 2, P, P, null) != 0
    assert "unknown flags" in _hip.last_error()
    assert lib.awq_group_params_ex(null, 0, 0, 128, 128, 4, 0, _hip.GP_TORCH_GPU, P, P, null) == 0
    assert lib.awq_dequant_ceiling(P, P, 24, null) != 0 and "multiple of 16" in _hip.last_error()
    assert lib.awq_dequant_ceiling(ctypes.c_void_p(66), P, 32, null) != 0 and "misaligned" in _hip.last_error()
    assert lib.awq_dequant_ceiling(null, null, 0, null) == 0


def test_cli_run_metrics_line():
    """The CLI's per-run JSON metrics line (main.run_metrics): the quantized tensors' input
    bytes over the run's wall time."""
    from awq_quantizer.main import run_metrics
    from awq_quantizer.model_loading.safetensors_loader import TensorInfo
    ordered = [TensorInfo("a", "f", torch.bfloat16, (4, 256)), TensorInfo("b", "f", torch.float16, (8,)),
               TensorInfo("c", "f", torch.float32, (2, 128))]
    m = run_metrics(ordered, {"a": {}, "c": {}}, {"quantize_s": 0.25, "total_s": 0.5})
    assert m["tensors"] == 2 and m["input_bytes"] == 4 * 256 * 2 + 2 * 128 * 4
    assert m["quantize_s"] == 0.25 and m["total_s"] == 0.5
    assert m["input_GB_per_s"] == round(m["input_bytes"] / 0.5 / 1e9, 3)
