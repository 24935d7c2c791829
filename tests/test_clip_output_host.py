"""CPU-only tests of the token-sample clip loss's host layer (include/awq_hip.h
awq_quantize_clip_output): the two C-ABI symbols are exported and bound, the entry
refuses what the header says before any pointer is looked at, the workspace formula, the
--clip_loss flag rules, quantize_layer_group's and quantize_block's clip_loss, and a numpy
restatement of the kernel's hi / lo bf16 split over one group."""
import ctypes

import numpy as np
import pytest
import torch

BF16, F16, F32, F64, I32 = 0, 1, 2, 3, 4   # include/awq_hip.h AWQ_DTYPE_*
OK, EINVAL, EUNSUPPORTED = 0, 1, 2
A = 4096                                   # a non-null, 16-B aligned address that is never dereferenced


def _lib():
    from awq_quantizer import _hip
    return _hip.load_library()


def _call(*, w=0, dtype=BF16, rows=4, K=256, gs=128, bits=4, sym=0, cs=0, rs=0, x=0, T=8, stride=None, n_grid=20, c0=0,
          nc=10, qweight=0, qzeros=0, scales=0, best=0, gloss=0, closs=0, lstride=0, work=0):
    """awq_quantize_clip_output, by default with NULL device pointers: every refusal comes first."""
    P = ctypes.c_void_p
    return _lib().awq_quantize_clip_output(P(w), dtype, rows, K, gs, bits, sym, P(cs), P(rs), P(x), T,
                                           K if stride is None else stride, n_grid, c0, nc, P(qweight), P(qzeros),
                                           P(scales), P(best), P(gloss), P(closs), lstride, P(work), None)


def test_symbols_exported_and_bound():
    from awq_quantizer import _hip
    lib = _lib()
    for name in ("awq_quantize_clip_output", "awq_quantize_clip_output_work_bytes", "awq_quantize_clip_output_fast"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert lib.awq_quantize_clip_output_work_bytes.restype is ctypes.c_int64
    assert len(_hip.SIGNATURES["awq_quantize_clip_output"][1]) == 24
    assert len(_hip.SIGNATURES["awq_quantize_clip_output_work_bytes"][1]) == 5
    assert lib.awq_abi_version() == 17          # additive symbols: the ABI number stays
    assert callable(_hip.quantize_clip_output)


def test_work_bytes():
    """Every loss is formed in registers: no workspace for any shape, `work` may be NULL."""
    lib = _lib()
    for args in ((4096, 4096, 128, 512, 10), (130, 96, 32, 300, 4), (1, 8, 8, 1, 1), (0, 0, 128, 0, 1),
                 (33, 1536, 512, 65, 10), (-1, 5, 128, 5, 1)):
        assert lib.awq_quantize_clip_output_work_bytes(*args) == 0, args


def test_fast_kernel_predicate():
    """awq_quantize_clip_output_fast, the predicate the entry routes by: bf16, group size 32 .. 256, 16-B
    aligned w / x / col_scale / col_rscale, x_row_stride % 8 == 0, K and the stride below 2^22."""
    P = ctypes.c_void_p

    def fast(w=A, dtype=BF16, K=256, gs=128, cs=A, rs=A, x=A, stride=256):
        return _lib().awq_quantize_clip_output_fast(P(w), dtype, K, gs, P(cs), P(rs), P(x), stride)

    assert fast() == 1 and fast(rs=0) == 1 and fast(stride=264) == 1 and fast(gs=32) == 1 and fast(gs=256) == 1
    for kw in (dict(dtype=F16), dict(dtype=F32), dict(gs=16), dict(gs=512, K=512), dict(w=A + 2), dict(x=A + 2),
               dict(cs=A + 4), dict(rs=A + 4), dict(stride=259), dict(K=1 << 22, stride=1 << 22),
               dict(stride=(1 << 22) + 8)):
        assert fast(**kw) == 0, kw


OUT = dict(best=A)     # one output, so that the later checks are reached
REFUSALS = [
    (dict(bits=3), EINVAL, "bit width"), (dict(bits=16), EINVAL, "bit width"),
    (dict(gs=0), EINVAL, "Group size"), (dict(gs=-8), EINVAL, "Group size"),
    (dict(rows=-1), EINVAL, "negative"), (dict(K=-256), EINVAL, "negative"), (dict(T=-1), EINVAL, "negative"),
    (dict(gs=4), EUNSUPPORTED, "power of two"), (dict(gs=96, K=192), EUNSUPPORTED, "power of two"),
    (dict(gs=1024, K=1024), EUNSUPPORTED, "power of two"),
    (dict(K=200), EUNSUPPORTED, "multiple"),                       # K % group_size
    (dict(dtype=F64), EUNSUPPORTED, "fp64"), (dict(dtype=I32), EINVAL, "dtype"), (dict(dtype=-1), EINVAL, "dtype"),
    (dict(stride=255), EINVAL, "x_row_stride"), (dict(stride=0), EINVAL, "x_row_stride"),
    (dict(nc=0), EINVAL, "n_candidates"), (dict(n_grid=0, nc=0), EINVAL, "n_candidates"),
    (dict(c0=-1), EINVAL, "cand_begin"), (dict(c0=11, nc=10), EINVAL, "n_grid"), (dict(nc=21), EINVAL, "n_grid"),
    (dict(c0=20, nc=1), EINVAL, "n_grid"),
    (dict(rows=1 << 40, K=1 << 30, gs=128), EUNSUPPORTED, "exceed"), (dict(rows=1 << 40, T=1 << 30), EUNSUPPORTED, "exceed"),
    (dict(rows=1 << 31, K=256), EUNSUPPORTED, "exceed"),           # rows * G >= 2^31
    (dict(), EINVAL, "no output"),                                 # a valid shape without any output
    (dict(**OUT), EINVAL, "null input"),                           # ... and with one: the NULL inputs
    (dict(w=A, cs=A, **OUT), EINVAL, "null input"),                # x with T > 0
    (dict(w=A, cs=A, x=A, gloss=A, lstride=7), EINVAL, "loss_stride"),
    (dict(w=A, cs=A, x=A, closs=A, lstride=7), EINVAL, "loss_stride"),
    (dict(w=A + 1, cs=A, x=A, **OUT), EINVAL, "aligned"), (dict(w=A, cs=A + 2, x=A, **OUT), EINVAL, "aligned"),
    (dict(w=A, cs=A, x=A + 1, **OUT), EINVAL, "aligned"), (dict(w=A, cs=A, x=A, scales=A + 1), EINVAL, "aligned"),
    (dict(w=A, cs=A, x=A, closs=A + 2, lstride=8), EINVAL, "aligned"),
]


def test_refusals_come_before_any_pointer_is_looked_at():
    from awq_quantizer import _hip
    for kw, code, word in REFUSALS:
        assert _call(**kw) == code, kw
        assert word in _hip.last_error(), (kw, _hip.last_error())


def test_refusal_order_follows_the_two_entries_it_is_built_from():
    """bits, group size, negative shapes, the group size's form, K % group_size, the dtype, the stride
    (awq_output_error's order), then the candidates (awq_quantize_clip_scaled's rule)."""
    from awq_quantizer import _hip
    order = [(dict(bits=3), "bit width"), (dict(rows=-1), "negative"), (dict(gs=96), "power of two"),
             (dict(K=200), "multiple"), (dict(dtype=F64), "fp64"), (dict(stride=1), "x_row_stride"),
             (dict(nc=0), "n_candidates"), (dict(), "no output")]
    for i in range(len(order)):              # everything from the i-th on is wrong: the i-th is reported
        kw = {}
        for later, _ in order[i:]:
            kw.update(later)
        assert _call(**kw) != OK
        assert order[i][1] in _hip.last_error(), (i, kw, _hip.last_error())


def test_empty_shapes_return_before_the_pointers():
    for kw in (dict(rows=0, **OUT), dict(K=0, **OUT)):
        assert _call(**kw) == OK, kw
    assert _call(rows=0) == EINVAL              # ... but still need an output


def test_python_wrapper_checks_its_buffers():
    from awq_quantizer import _hip
    w = torch.zeros(2, 256, dtype=torch.bfloat16)
    v = torch.ones(256)
    x = torch.zeros(3, 256, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="samples"):
        _hip.quantize_clip_output(w, v, x[:, :128], 128, 4, False, 20, 10)
    with pytest.raises(ValueError, match="samples"):
        _hip.quantize_clip_output(w, v, x.float(), 128, 4, False, 20, 10)
    for bad in (torch.zeros(2, 3), torch.zeros(3, 4), torch.zeros(2, 4, dtype=torch.float64)):
        with pytest.raises(ValueError, match="group_loss"):
            _hip.quantize_clip_output(w, v, x, 128, 4, False, 20, 10, group_loss=bad)
    with pytest.raises(ValueError, match="cand_loss"):
        _hip.quantize_clip_output(w, v, x, 128, 4, False, 20, 10, cand_loss=torch.zeros(9, 4))
    with pytest.raises(ValueError, match="cand_loss"):     # one stride for both
        _hip.quantize_clip_output(w, v, x, 128, 4, False, 20, 10, group_loss=torch.zeros(2, 4),
                                  cand_loss=torch.zeros(10, 5))
    with pytest.raises(ValueError, match="group_loss"):
        _hip.quantize_clip_output(w, v, x, 128, 4, False, 20, 10, group_loss=torch.zeros(2, 4), loss_offset=1)


# ---------------------------------------------------------------- the CLI's flags
BASE = ["--model_id", "m", "--output_dir", "o"]
FOLD = ["--scale_method", "awq", "--output_format", "autoawq", "--fold_scales"]


def test_clip_loss_flag_rules():
    from awq_quantizer.options import check_flags, parse_args
    assert parse_args(BASE).clip_loss == "diag"
    clip = FOLD + ["--act_clip", "--clip_loss", "output"]
    ok = [FOLD + ["--act_stats", "s", "--act_clip"], FOLD + ["--act_stats", "s", "--act_clip", "--clip_loss", "diag"],
          FOLD + ["--act_stats", "s", "--clip_loss", "diag"],
          clip + ["--act_stats", "s", "--act_samples", "x"],            # --act_samples for the clip loss alone
          clip + ["--calib_ids", "ids"], clip + ["--calib_ids", "ids", "--n_sample_tokens", "64"],
          clip + ["--act_stats", "s", "--act_samples", "x", "--search_loss", "output"],
          clip + ["--calib_ids", "ids", "--search_loss", "output"]]
    for argv in ok:
        assert check_flags(parse_args(BASE + argv)) is None, argv
    bad = {"--clip_loss output needs --act_clip": FOLD + ["--act_stats", "s", "--clip_loss", "output", "--act_samples", "x"],
           "--clip_loss output needs --fold_scales": ["--scale_method", "awq", "--act_stats", "s", "--output_format",
                                                      "packed", "--act_clip", "--clip_loss", "output", "--act_samples", "x"],
           "--clip_loss output needs token samples": clip + ["--act_stats", "s"],
           "one of them": clip + ["--calib_ids", "ids", "--act_samples", "x"],
           "--n_sample_tokens must be positive": clip + ["--calib_ids", "ids", "--n_sample_tokens", "0"],
           # today's messages, verbatim, for today's combinations
           "--act_samples is read by --search_loss output": FOLD + ["--act_stats", "s", "--act_clip", "--act_samples", "x"],
           "--search_loss output needs token samples": FOLD + ["--act_stats", "s", "--search_loss", "output"]}
    for want, argv in bad.items():
        err = check_flags(parse_args(BASE + argv))
        assert err is not None and want in err, (want, err)
    with pytest.raises(SystemExit):
        parse_args(BASE + ["--clip_loss", "mse"])


def test_missing_samples_file_is_an_error_before_the_model_is_read(tmp_path, capsys):
    """The message names the flag and the file; nothing about the (missing) model or a device is
    logged before it."""
    from awq_quantizer import main
    missing = str(tmp_path / "none")
    argv = ["--model_id", str(tmp_path / "no_such_model"), "--output_dir", str(tmp_path / "o"), "--log_level",
            "ERROR"] + FOLD + ["--act_stats", "s", "--act_clip", "--clip_loss", "output", "--act_samples", missing]
    assert main.main(argv) == 1
    errors = [line for line in capsys.readouterr().out.splitlines() if " - ERROR - " in line]
    assert len(errors) == 1 and f"--act_samples: {missing} does not exist" in errors[0], errors


# ---------------------------------------------------------------- the Python API's argument rules
def _quantizer(**kw):
    from awq_quantizer.quantization import AWQQuantizer
    return AWQQuantizer(**dict(dict(bits=4, group_size=128, symmetric=False, scale_method="awq", device="cuda:0",
                                    logger_level="CRITICAL"), **kw))


def test_layer_group_clip_loss_argument_errors():
    from awq_quantizer.quantization import AWQQuantizer, act_search
    w = {"a": torch.zeros(4, 256, dtype=torch.bfloat16)}
    v = torch.ones(256)
    q = _quantizer()
    assert AWQQuantizer.clip_loss == "diag" and q.clip_loss == "diag"
    with pytest.raises(ValueError, match="clip_loss='output' needs token samples"):
        act_search.quantize_layer_group(q, w, x_mean=v, x_sq=v, clip=True, clip_loss="output")
    with pytest.raises(ValueError, match="clip_loss must be"):
        act_search.quantize_layer_group(q, w, x_mean=v, x_sq=v, clip=True, clip_loss="mse")
    q.clip_loss = "output"                      # the methods read the quantizer's setting
    with pytest.raises(ValueError, match="clip_loss='output' needs token samples"):
        q.quantize_layer_group(w, x_mean=v, x_sq=v, clip=True)
    q.clip_loss = "mse"
    with pytest.raises(ValueError, match="clip_loss must be"):
        q.quantize_layer_group(w, x_mean=v, x_sq=v, clip=True)
    with pytest.raises(ValueError, match="clip_loss must be"):
        q.quantize_block({}, {}, None, clip=True)


def test_quantize_block_passes_clip_loss_through(monkeypatch):
    """Stub ops: each group's samples and clip_loss reach quantize_layer_group; a group without
    samples falls back to the diagonal clip with a warning."""
    from awq_quantizer.quantization import act_search
    from awq_quantizer.quantization.block_plan import Block, Group
    q = _quantizer(group_size=32)
    monkeypatch.setattr(q, "_check_mode", lambda: None)
    monkeypatch.setattr(q, "compute_device", lambda: torch.device("cpu"))
    calls, warnings = [], []
    monkeypatch.setattr(q.logger, "warning", lambda msg: warnings.append(msg))

    def stub(qq, weights, activations=None, **kw):
        # (the default choice travels through AWQQuantizer.quantize_layer_group, which names every
        #  keyword and leaves clip_loss to the quantizer's attribute: one view of both routes)
        kw = {k: v for k, v in kw.items() if v is not None}
        kw.setdefault("clip_loss", qq.clip_loss)
        calls.append((list(weights), kw))
        K = next(iter(weights.values())).shape[1]
        return {"results": {n: {"qweight": torch.zeros(1), "input_scale": torch.ones(K)} for n in weights},
                "input_scale": torch.ones(K), "ratio": 0.0, "best": 0, "losses": None,
                "clip": {"loss_before": 2.0, "loss_after": 1.0, "loss": kw["clip_loss"]}}

    monkeypatch.setattr(act_search, "quantize_layer_group", stub)
    names = {"attn_out": "L.self_attn.o_proj.weight", "mlp_out": "L.mlp.down_proj.weight"}
    block = Block("L", {g: Group(g, [n], [], "rows", False, "stub") for g, n in names.items()})
    tensors = {n: torch.zeros(4, 64, dtype=torch.bfloat16) for n in names.values()}
    stats = {n: (torch.ones(64), torch.ones(64)) for n in names.values()}
    smp = {"attn_out": torch.zeros(3, 64, dtype=torch.bfloat16)}
    out = act_search.quantize_block(q, tensors, stats, block, clip=True, samples=smp, clip_loss="output")
    by_group = {c[0][0]: c[1] for c in calls}
    a, m = by_group[names["attn_out"]], by_group[names["mlp_out"]]
    assert a["clip_loss"] == "output" and a["samples"] is smp["attn_out"] and a["clip"] is True
    assert m["clip_loss"] == "diag" and "samples" not in m
    assert a.get("loss", "diag") == "diag" and m.get("loss", "diag") == "diag"   # the scale search keeps its loss
    assert len(warnings) == 1 and "mlp_out" in warnings[0] and "clip_loss='output'" in warnings[0]
    assert out["groups"]["attn_out"]["clip"]["loss"] == "output"
    # the default, and the quantizer's own setting through the method
    calls.clear()
    act_search.quantize_block(q, tensors, stats, block, clip=True, samples=smp)
    assert [c[1]["clip_loss"] for c in calls] == ["diag", "diag"] and all("samples" not in c[1] for c in calls)
    calls.clear()
    q.clip_loss = "output"
    q.quantize_block(tensors, stats, block, clip=True, samples=smp)
    assert sorted(c[1]["clip_loss"] for c in calls) == ["diag", "output"]
    calls.clear()
    monkeypatch.setattr(q, "quantize_packed", lambda w: {"qweight": torch.zeros(1)})
    q.quantize_block(tensors, stats, block, samples=smp)         # without clip=True there is no clip search
    assert calls == []
    # an override of the method is still what quantize_block calls for the default choice
    q.clip_loss = "diag"
    seen = []
    monkeypatch.setattr(q, "quantize_layer_group", lambda weights, **kw: (seen.append(list(weights)), stub(q, weights, **kw))[1])
    act_search.quantize_block(q, tensors, stats, block, clip=True)
    assert sorted(seen) == sorted([n] for n in names.values())


# ---------------------------------------------------------------- the hi / lo split over one group, restated in numpy
def rn_bf16(a: np.ndarray) -> np.ndarray:
    """round-to-nearest-even of float32 to bf16, returned as float32 (finite inputs)"""
    u = a.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("L", [32, 256])
def test_split_error_over_one_group_stays_under_eps_l(L):
    """d_hi + d_lo is within 2^-17 |d| of d per element; with an fp32 accumulation of the 2 L exact
    products on top, E of one group stays inside eps_L = 2^-17 + L 2^-22 of A = sum |d| |x|."""
    rng = np.random.default_rng(L)
    d = (rng.standard_normal((64, L)) * 0.01).astype(np.float32)
    x = rn_bf16(rng.standard_normal((48, L)).astype(np.float32))
    hi = rn_bf16(d)
    lo = rn_bf16((d - hi).astype(np.float32))
    s = hi.astype(np.float64) + lo.astype(np.float64)
    assert np.all(np.abs(s - d) <= 2.0 ** -17 * np.abs(d))
    A = np.abs(d).astype(np.float64) @ np.abs(x).astype(np.float64).T
    exact = d.astype(np.float64) @ x.astype(np.float64).T
    acc = np.zeros((64, 48), dtype=np.float32)
    for k in range(L):                                              # hi and lo of every k in turn, fp32 adds
        acc = (acc + hi[:, k:k + 1] * x[:, k][None, :]).astype(np.float32)
        acc = (acc + lo[:, k:k + 1] * x[:, k][None, :]).astype(np.float32)
    eps = 2.0 ** -17 + L * 2.0 ** -22
    rel = float((np.abs(acc.astype(np.float64) - exact) / A).max())
    print(f"split + fp32 accumulation, L = {L}: max error {rel:.2e} A (eps_L = {eps:.2e})")
    assert rel <= eps
