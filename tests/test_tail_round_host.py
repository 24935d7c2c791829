"""GPTQ error-compensated rounding without a GPU: the C entry's refusals with NULL
pointers, the flag rules, quantize_gptq's argument errors, and the NumPy restatement the GPU tests
compare against (tests/gptq_round_ref.py), whose compensated output error must be below
round-to-nearest's on the issue's inputs."""
import numpy as np
import pytest
import torch

import gptq_round_ref as gr

EINVAL, EUNSUPPORTED = 1, 2


def _lib():
    from awq_quantizer import _hip
    return _hip, _hip.load_library()


def _call(lib, N, K, gs, bits, sym, c0, n):
    return lib.awq_gptq_round_block(None, N, K, gs, bits, sym, None, c0, n, None, None, None, None, None)


def test_symbol_is_exported_and_bound():
    _hip, lib = _lib()
    assert "awq_gptq_round_block" in _hip.SIGNATURES and hasattr(lib, "awq_gptq_round_block")
    assert lib.awq_abi_version() == 17 == _hip.ABI_VERSION
    assert callable(_hip.gptq_round_block) and _hip.GPTQ_BLOCK == 128


REFUSED = [
    # (N, K, gs, bits, sym, col_begin, n_cols) -> code, a piece of the message
    ((8, 256, 128, 3, 0, 0, 128), EUNSUPPORTED, "bit width"),
    ((8, 256, 128, 16, 0, 0, 128), EUNSUPPORTED, "bit width"),
    ((8, 256, 128, 4, 2, 0, 128), EINVAL, "symmetric"),
    ((8, 256, 16, 4, 0, 0, 128), EUNSUPPORTED, "group_size 32, 64 or 128"),
    ((8, 256, 256, 4, 0, 0, 128), EUNSUPPORTED, "group_size 32, 64 or 128"),
    ((8, 256, 0, 4, 0, 0, 128), EUNSUPPORTED, "group_size 32, 64 or 128"),
    ((8, 200, 64, 4, 0, 0, 64), EINVAL, "multiple of group_size"),
    ((8, 512, 128, 4, 0, 0, 256), EINVAL, "n_cols"),
    ((8, 256, 64, 4, 0, 0, 96), EINVAL, "n_cols"),
    ((8, 256, 128, 4, 0, 0, 64), EINVAL, "n_cols"),
    ((8, 256, 32, 4, 0, 16, 32), EINVAL, "col_begin"),
    ((8, 256, 64, 4, 0, 32, 64), EINVAL, "col_begin"),
    ((8, 256, 128, 4, 0, 256, 128), EINVAL, "col_begin"),
    ((8, 256, 128, 4, 0, 384, 0), EINVAL, "col_begin"),
    ((8, 192, 64, 4, 0, 128, 128), EINVAL, "col_begin"),
    ((-1, 256, 128, 4, 0, 0, 128), EINVAL, "negative"),
    ((8, -256, 128, 4, 0, 0, 128), EINVAL, "negative"),
    ((8, 256, 128, 4, 0, -128, 128), EINVAL, "negative"),
    ((8, 256, 128, 4, 0, 0, -128), EINVAL, "negative"),
    ((2 ** 31, 256, 128, 4, 0, 0, 128), EUNSUPPORTED, "2^31"),
    ((8, 256, 128, 4, 0, 0, 128), EINVAL, "null argument"),          # a valid shape, no buffers
    ((8, 256, 32, 8, 1, 128, 96), EINVAL, "null argument"),
]


@pytest.mark.parametrize("args,code,piece", REFUSED, ids=[str(a) for a, _, _ in REFUSED])
def test_refusals_come_before_any_pointer_is_looked_at(args, code, piece):
    _hip, lib = _lib()
    assert _call(lib, *args) == code
    assert piece in _hip.last_error(), _hip.last_error()


@pytest.mark.parametrize("args", [(0, 256, 128, 4, 0, 0, 128), (8, 0, 128, 4, 0, 0, 0), (8, 256, 64, 8, 1, 128, 0),
                                  (8, 256, 64, 8, 1, 256, 0)], ids=str)
def test_empty_shapes_return_0(args):
    _hip, lib = _lib()
    assert _call(lib, *args) == 0 and _hip.last_error() == ""


def test_misaligned_buffers_are_refused():
    """Host pointers stand in for device memory: the entry refuses before anything is launched."""
    import ctypes
    _hip, lib = _lib()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 255) & ~255
    p = lambda off: ctypes.c_void_p(base + off)
    ok = [p(0), p(256), p(512), p(1024), p(1280), p(1536)]          # work, u, err, qweight, qzeros, scales
    for which, off in ((0, 4), (1, 8), (2, 4), (3, 2), (4, 1), (5, 1)):
        a = list(ok)
        a[which] = p(256 * which + off) if which < 3 else p(1024 + 256 * (which - 3) + off)
        rc = lib.awq_gptq_round_block(a[0], 8, 256, 128, 4, 0, a[1], 0, 128, a[2], a[3], a[4], a[5], None)
        assert rc == EINVAL and "aligned" in _hip.last_error(), (which, _hip.last_error())


# ---------------------------------------------------------------- flags
FOLD = ["--model_id", "m", "--output_dir", "o", "--scale_method", "awq", "--fold_scales", "--output_format", "autoawq"]


def test_flag_rules():
    from awq_quantizer.options import check_flags, parse_args
    a = parse_args(["--model_id", "m", "--output_dir", "o"])
    assert (a.rounding, a.gptq_damp) == ("nearest", 0.01) and check_flags(a) is None
    gptq = ["--rounding", "gptq"]
    ok = [FOLD + ["--act_stats", "s", "--act_samples", "x"] + gptq,
          FOLD + ["--calib_ids", "ids"] + gptq,
          FOLD[:-1] + ["gptq", "--symmetric", "--calib_ids", "ids", "--gptq_damp", "0.05"] + gptq,
          FOLD + ["--calib_ids", "ids", "--search_loss", "output"] + gptq]
    for argv in ok:
        assert check_flags(parse_args(argv)) is None, argv
    bad = {"--rounding gptq needs --fold_scales": ["--model_id", "m", "--output_dir", "o"] + gptq,
           "--rounding gptq needs token samples": FOLD + ["--act_stats", "s"] + gptq,
           "one of them": FOLD + ["--calib_ids", "ids", "--act_samples", "x"] + gptq,
           "--n_sample_tokens must be positive": FOLD + ["--calib_ids", "ids", "--n_sample_tokens", "0"] + gptq,
           "--rounding gptq refuses --act_clip": FOLD + ["--calib_ids", "ids", "--act_clip"] + gptq,
           "--gptq_damp must be in (0, 1)": FOLD + ["--calib_ids", "ids", "--gptq_damp", "0"] + gptq,
           # the existing rule stands: samples nobody reads
           "--act_samples is read by --search_loss output": FOLD + ["--act_stats", "s", "--act_samples", "x"]}
    for piece, argv in bad.items():
        err = check_flags(parse_args(argv))
        assert err is not None and piece in err, (piece, err)
    with pytest.raises(SystemExit):
        parse_args(["--model_id", "m", "--output_dir", "o", "--rounding", "stochastic"])


# ---------------------------------------------------------------- argument errors (before any device work)
def _quantizer(**kw):
    from awq_quantizer.quantization import AWQQuantizer
    return AWQQuantizer(bits=4, group_size=128, symmetric=False, device="cpu", logger_level="ERROR", **kw)


def test_quantize_gptq_argument_errors():
    q = _quantizer()
    w, x = torch.zeros(8, 256, dtype=torch.bfloat16), torch.zeros(16, 256, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="needs token samples"):
        q.quantize_gptq(w)
    with pytest.raises(ValueError, match=r"samples must be \[tokens, 256\]"):
        q.quantize_gptq(w, x[:, :128])
    with pytest.raises(ValueError, match=r"hessian must be \[256, 256\]"):
        q.quantize_gptq(w, hessian=torch.zeros(128, 128))
    for damp in (0, -0.01, 1.0, float("nan"), "0.01", True):
        with pytest.raises(ValueError, match="damp must be a number in"):
            q.quantize_gptq(w, x, damp=damp)
    with pytest.raises(ValueError, match="input_scale must have in_features"):
        q.quantize_gptq(w, x, input_scale=torch.ones(128))
    with pytest.raises(ValueError, match="2-D"):
        q.quantize_gptq(w.reshape(-1), x)
    with pytest.raises(ValueError, match="group_size in"):
        q.quantize_gptq(torch.zeros(8, 192, dtype=torch.bfloat16), torch.zeros(4, 192, dtype=torch.bfloat16))
    from awq_quantizer.quantization import AWQQuantizer
    q256 = AWQQuantizer(bits=4, group_size=256, symmetric=False, device="cpu", logger_level="ERROR")
    with pytest.raises(ValueError, match="group_size in"):
        q256.quantize_gptq(w, x)


def test_rounding_attribute_and_clip():
    from awq_quantizer.quantization import AWQQuantizer
    assert AWQQuantizer.rounding == "nearest" and AWQQuantizer.gptq_damp == 0.01
    q = _quantizer(scale_method="awq")
    assert q.rounding == "nearest"
    w = {"w": torch.zeros(8, 256, dtype=torch.bfloat16)}
    st = torch.ones(256)
    q.rounding = "gptq"
    with pytest.raises(ValueError, match="clip=True with rounding='gptq'"):
        q.quantize_layer_group(w, x_mean=st, x_sq=st, clip=True)
    with pytest.raises(ValueError, match="packed outputs only"):
        q.quantize_layer_group(w, x_mean=st, x_sq=st, packed=False)
    with pytest.raises(ValueError, match="clip=True with rounding='gptq'"):
        q.quantize_block({}, {}, None, clip=True)            # (refused before the block is looked at)
    q.rounding = "stochastic"
    with pytest.raises(ValueError, match="rounding must be"):
        q.quantize_layer_group(w, x_mean=st, x_sq=st)


# ---------------------------------------------------------------- the restatement
CASES = [(32, 256, 512, 128), (32, 256, 128, 128), (32, 256, 512, 32), (16, 384, 300, 64)]


@pytest.mark.parametrize("N,K,T,gs", CASES, ids=str)
def test_restatement_beats_round_to_nearest(N, K, T, gs):
    """4-bit asymmetric on the issue's correlated inputs: the compensated output error is below
    round-to-nearest's, in float32 and in float64, and the two runs' losses agree closely."""
    for seed in range(2):
        X, W = gr.inputs(N, K, T, seed)
        W32 = W.astype(np.float32)
        U, dead = gr.factor(X)
        assert not dead.any()
        rtn = gr.solve(W32, U, gs, 4, False, propagate=False)
        got = gr.solve(W32, U, gs, 4, False)
        ref = gr.solve(W32, U, gs, 4, False, dtype=np.float64)
        l_rtn, l32, l64 = (gr.output_loss(gr.dequantize(r, gs), W32, X) for r in (rtn, got, ref))
        print(f"N {N} K {K} T {T} gs {gs} seed {seed}: loss / loss_rtn {l32 / l_rtn:.4f} (float64 {l64 / l_rtn:.4f})")
        assert l32 < l_rtn and l64 < l_rtn
        assert abs(l32 / l64 - 1) < 0.05
        # round-to-nearest with the same rule is the project's RTN: the oracle's fields of the fp32 weight
        from oracle import awq_oracle as orc
        tq, sc, zp = orc.quantize_groups(torch.from_numpy(W32), N, K, gs, 4, False)
        assert np.array_equal(sc.view(torch.int16).numpy().astype(np.uint16), rtn["sbits"])
        assert np.array_equal(zp.numpy(), rtn["zfields"])


def test_restatement_special_rows():
    """A constant group, an all-zero group and a NaN: the row's fields follow the existing semantics,
    nothing is propagated out of such a group, and the other rows do not change."""
    X, W = gr.inputs(8, 256, 300, 3)
    U, _ = gr.factor(X)
    W32 = W.astype(np.float32)
    base = gr.solve(W32, U, 128, 4, False)
    V = W32.copy()
    V[1, :128] = 0.25
    V[2, :128] = 0.0
    V[3, 130] = np.nan
    got = gr.solve(V, U, 128, 4, False)
    keep = [0, 4, 5, 6, 7]
    for k in ("fields", "zfields", "sbits"):
        assert np.array_equal(got[k][keep], base[k][keep]), k
    assert (got["fields"][2, :128] == 0).all() and got["zfields"][2, 0] == 0 and got["sbits"][2, 0] == 0
    assert got["sbits"][1, 0] == 0 and (got["fields"][1, :128] == 15).all()        # scale 1e-10 -> fp16 0: q = qmax
    work = V.copy()                                                                # nothing leaves such a group
    scratch = {k: v.copy() for k, v in got.items()}
    err = gr.round_block(work, U.astype(np.float32), 128, 4, False, 0, 128, scratch["fields"], scratch["zfields"],
                         scratch["sbits"])
    assert not err[1:3].any() and np.array_equal(work[1:3], V[1:3]) and err[0].any()
    assert got["sbits"][3, 1] == 0xFFFF and (got["fields"][3, 128:] == 0).all() and got["zfields"][3, 1] == 0
    assert np.array_equal(got["fields"][3, :128], gr.solve(V[3:4], U, 128, 4, False)["fields"][0, :128])
