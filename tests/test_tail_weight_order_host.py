"""GPTQ act-order without a GPU: the flag's rules, what import_gptq and
export_autoawq refuse before any device work, verify's findings, and the entries' argument checks."""
import pytest
import torch

import gptq_layout as gl


def test_flag_rules():
    from awq_quantizer.options import ACT_ORDER_NEEDS, check_flags, parse_args
    base = ["--model_id", "m", "--output_dir", "o", "--scale_method", "awq", "--fold_scales", "--act_stats", "s",
            "--act_samples", "a"]
    ok = base + ["--rounding", "gptq", "--output_format", "gptq", "--gptq_act_order"]
    assert check_flags(parse_args(ok)) is None and parse_args(ok).gptq_act_order is True
    assert parse_args(base).gptq_act_order is False
    for bad in (base + ["--output_format", "gptq", "--gptq_act_order"],
                base + ["--rounding", "gptq", "--output_format", "autoawq", "--gptq_act_order"]):
        assert check_flags(parse_args(bad)) == ACT_ORDER_NEEDS
    assert "--rounding gptq" in ACT_ORDER_NEEDS and "--output_format gptq" in ACT_ORDER_NEEDS


def _linear(N=8, K=64, gs=32):
    g = torch.Generator().manual_seed(3)
    return gl.pack(torch.randint(0, 16, (N, K), generator=g), torch.randint(0, 16, (N, K // gs), generator=g),
                   torch.rand(N, K // gs, generator=g).half(), gs, 1)


def test_refusals_come_before_any_device_work():
    from awq_quantizer.quantization import AWQQuantizer
    from awq_quantizer.verify import gptq_findings
    q = AWQQuantizer(bits=4, group_size=32, symmetric=False, device="cpu", logger_level="ERROR")
    t = _linear()
    unbalanced = t["g_idx"].clone()
    unbalanced[40] = 0
    with pytest.raises(ValueError, match=r"act-order, desc_act = true, is not supported"):
        q.import_gptq(dict(t, g_idx=unbalanced))
    with pytest.raises(ValueError, match="g_idx must hold 64 group indices"):
        q.dequantize_gptq(dict(t, g_idx=torch.full((64,), 2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="no AutoAWQ GEMM form"):
        q.export_autoawq({"perm": torch.arange(64, dtype=torch.int32)})
    balanced = t["g_idx"].flip(0)
    word = "act-order (desc_act) checkpoints are not supported"
    assert gptq_findings(dict(t, g_idx=balanced), 32, False, "gptq", desc_act=True) == []
    assert word in gptq_findings(dict(t, g_idx=balanced), 32, False, "gptq")[0]
    found = gptq_findings(dict(t, g_idx=unbalanced), 32, False, "gptq", desc_act=True)
    assert found == [f"g_idx[40] = 0, not 1 = k // group_size at 1 position(s): {word}"]


@pytest.mark.parametrize("call,code,word", [
    (lambda l, p: l.awq_gptq_permute_rows(p, p, 8, 12, p, None), 1, "% 8"),
    (lambda l, p: l.awq_gptq_permute_rows(p, p, 8, 64, p, None), 1, "not in place"),
    (lambda l, p: l.awq_gptq_permute_rows(None, None, 0, 64, None, None), 0, ""),
    (lambda l, p: l.awq_gptq_gidx_from_perm(p, 64, 0, p, p, None), 1, "Group size"),
    (lambda l, p: l.awq_gptq_gidx_from_perm(p, 64, 32, None, None, None), 1, "at least one output"),
    (lambda l, p: l.awq_gptq_check_index(p, 4, -1, p, None), 1, "negative"),
    (lambda l, p: l.awq_dequantize_gptq(p, p, p, p, 8, 64, 2, 2, p, 2, None), 1, "zero_offset"),
    (lambda l, p: l.awq_dequantize_gptq(p, p, p, p, 8, 64, 2, 1, p, 3, None), 2, "fp32, fp16 or bf16"),
    (lambda l, p: l.awq_dequantize_gptq(p, p, p, p, 8, 64, 0, 1, p, 2, None), 1, "at least one group"),
    (lambda l, p: l.awq_dequantize_gptq(p, p, p, None, 8, 64, 2, 1, p, 2, None), 1, "null"),
])
def test_entries_refuse_without_a_launch(call, code, word):
    import ctypes
    from awq_quantizer import _hip
    lib = _hip.load_library()
    assert lib.awq_abi_version() == 17
    buf = (ctypes.c_char * 64)()
    assert call(lib, ctypes.cast(buf, ctypes.c_void_p)) == code and word in _hip.last_error()
