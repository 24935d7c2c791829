"""awq_gptq_factor without a GPU: the argument checks in their documented order with
pointers never dereferenced, the workspace size, --gptq_factor's rules, q.gptq_factor's validation."""
import ctypes

import pytest
import torch

EINVAL, EUNSUPPORTED = 1, 2


def _lib():
    from awq_quantizer import _hip
    return _hip, _hip.load_library()


def test_symbols_and_workspace():
    _hip, lib = _lib()
    assert lib.awq_abi_version() == 17 == _hip.ABI_VERSION and callable(_hip.gptq_factor)
    for name in ("awq_gptq_factor", "awq_gptq_factor_workspace"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    # one double per diagonal block of 128
    assert [lib.awq_gptq_factor_workspace(K) for K in (-1, 0, 1, 128, 192, 14336)] == [0, 0, 8, 8, 16, 896]
    assert lib.awq_gptq_factor(None, 0, 0.01, None, 0, None, None) == 0 and _hip.last_error() == ""     # K == 0


_BUF = (ctypes.c_char * 1024)()
_BASE = (ctypes.addressof(_BUF) + 255) & ~255
P = lambda off: ctypes.c_void_p(_BASE + off)          # host memory stands in: the entry refuses before any launch
OK = dict(h=P(0), K=256, damp=0.01, ws=P(256), nbytes=16, status=P(512))

# in the documented order: each case also carries a fault that is checked later
REFUSED = [
    (dict(K=-1, damp=2.0, h=None), EINVAL, "negative"), (dict(damp=0.0, h=None), EINVAL, "damp"),
    (dict(damp=1.0, K=2 ** 31), EINVAL, "damp"), (dict(damp=float("nan")), EINVAL, "damp"),
    (dict(damp=float("inf")), EINVAL, "damp"), (dict(K=2 ** 31, h=None), EUNSUPPORTED, "2^42"),
    (dict(K=2 ** 21, h=None), EUNSUPPORTED, "2^42"), (dict(K=200, h=None), EUNSUPPORTED, "multiple of 32"),
    (dict(h=None, nbytes=0), EINVAL, "null argument"), (dict(ws=None, nbytes=0), EINVAL, "null argument"),
    (dict(status=None, h=P(4)), EINVAL, "null argument"), (dict(h=P(4), nbytes=0), EINVAL, "aligned"),
    (dict(ws=P(260), nbytes=0), EINVAL, "aligned"), (dict(status=P(514), nbytes=0), EINVAL, "aligned"),
    (dict(nbytes=15), EINVAL, "workspace"),
]


@pytest.mark.parametrize("change,code,piece", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refusals_in_order(change, code, piece):
    _hip, lib = _lib()
    a = dict(OK, **change)
    assert lib.awq_gptq_factor(a["h"], a["K"], a["damp"], a["ws"], a["nbytes"], a["status"], None) == code
    assert piece in _hip.last_error(), _hip.last_error()


FOLD = ["--model_id", "m", "--output_dir", "o", "--scale_method", "awq", "--fold_scales", "--output_format", "autoawq",
        "--calib_ids", "ids"]


def test_flag_rules():
    from awq_quantizer.options import check_flags, parse_args
    a = parse_args(["--model_id", "m", "--output_dir", "o"])
    assert a.gptq_factor == "torch" and check_flags(a) is None
    assert parse_args(FOLD + ["--rounding", "gptq"]).gptq_factor == "torch"
    assert check_flags(parse_args(FOLD + ["--rounding", "gptq", "--gptq_factor", "hip"])) is None
    err = check_flags(parse_args(FOLD + ["--gptq_factor", "hip"]))
    assert err is not None and "--gptq_factor is read by --rounding gptq" in err
    with pytest.raises(SystemExit):
        parse_args(FOLD + ["--rounding", "gptq", "--gptq_factor", "lapack"])


def test_quantizer_attribute():
    from awq_quantizer.quantization import AWQQuantizer
    assert AWQQuantizer.gptq_factor == "torch"
    q = AWQQuantizer(bits=4, group_size=128, symmetric=False, device="cpu", logger_level="ERROR")
    q.gptq_factor = "lapack"
    with pytest.raises(ValueError, match="gptq_factor must be one of"):
        q.quantize_gptq(torch.zeros(8, 256, dtype=torch.bfloat16), torch.zeros(16, 256, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="contiguous float32"):
        from awq_quantizer import _hip
        _hip.gptq_factor(torch.zeros(4, 4), 0.01)
