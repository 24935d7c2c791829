"""GPTQ-layout checkpoints, the parts that need no GPU: the CPU restatement of the layout
(tests/gptq_layout.py) and its cross-check against the oracle's quantize through an independent
dequantize; the refusals of awq_export_gptq / awq_import_gptq in their documented order
(include/awq_hip.h; nothing is launched, pointers are never dereferenced); the CLI's flag rules for
--output_format gptq; the writer's files on a tiny model with CPU-made results; verify's findings
on hand-altered directories."""
import json

import pytest
import torch
from safetensors.torch import load_file, save_file

import gptq_layout as gl
from oracle import awq_oracle as orc

OK, EINVAL, EUNSUPPORTED = 0, 1, 2


# ---------------------------------------------------------------- the helper
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("N,K,gs", [(8, 32, 32), (24, 160, 32), (16, 576, 64)])
def test_helper_round_trip(N, K, gs, off):
    g = torch.Generator().manual_seed(N + K + off)
    G = K // gs
    u = torch.randint(0, 16, (N, K), generator=g)
    z = torch.randint(0, 16, (N, G), generator=g)
    z[0, 0], z[1, 0], z[2, 0] = 0, 1, 15
    sc = torch.randint(-2 ** 15, 2 ** 15, (N, G), generator=g, dtype=torch.int16).view(torch.float16)
    t = gl.pack(u, z, sc, gs, off)
    assert t["qweight"].shape == (K // 8, N) and t["qzeros"].shape == (G, N // 8)
    assert t["scales"].shape == (G, N) and t["g_idx"].tolist() == [k // gs for k in range(K)]
    # the table, element by element
    for (n, k) in ((0, 0), (N - 1, K - 1), (3, 9), (5, K // 2 + 3)):
        assert (int(t["qweight"][k // 8, n]) >> (4 * (k % 8))) & 15 == int(u[n, k])
    for (n, gg) in ((0, 0), (1, 0), (2, 0), (N - 1, G - 1)):
        assert (int(t["qzeros"][gg, n // 8]) >> (4 * (n % 8))) & 15 == (int(z[n, gg]) - off) & 15
    u2, z2, s2 = gl.unpack(t, off)
    assert torch.equal(u2, u) and torch.equal(z2, z) and torch.equal(s2.view(torch.int16), sc.view(torch.int16))
    # the row-major words: pad fields of a row's last qzeros word are 0
    w = gl.to_packed_words(t, off)
    assert torch.equal(w["qweight"], orc.pack_rows(u.to(torch.int32), 4, 0))
    assert torch.equal(w["qzeros"], orc.pack_rows(z.to(torch.int32), 4, 0))
    assert w["qzeros"].shape == (N, -(-G // 8))


@pytest.mark.parametrize("fmt", ["gptq", "gptq_v2"])
@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
def test_helper_dequantize_equals_the_oracle(sym, fmt):
    """The oracle's quantize -> fields -> the helper's pack -> the published GPTQ formula must be the
    oracle's own dequantize bit for bit: the symmetric fields are q + 8 with zero 8."""
    N, K, gs = 24, 160, 32
    x = (torch.randn(N, K, generator=torch.Generator().manual_seed(5)) * 0.02).bfloat16()
    ref = orc.quantize(x, bits=4, group_size=gs, symmetric=sym)
    qmin = orc.qrange(4, sym)[0]
    u, z = ref["tensor_q"].to(torch.int64) - qmin, ref["zero_points"].to(torch.int64) - qmin
    assert u.min() >= 0 and u.max() <= 15 and z.min() >= 0 and z.max() <= 15
    if sym:
        assert bool((z == 8).all())
    dq = gl.dequantize(gl.pack(u, z, ref["scales"], gs, gl.ZERO_OFFSET[fmt]), gl.ZERO_OFFSET[fmt])
    assert torch.equal(dq.view(torch.int32), orc.dequantize(ref).view(torch.int32))


# ---------------------------------------------------------------- the C calls
def _calls():
    from awq_quantizer import _hip
    lib = _hip.load_library()
    one = 0x1000                                                     # never dereferenced: refused first

    def export(N, K, gs, bits=4, sym=0, off=1, ins=(one, one, one), outs=(one, one, one, one)):
        return lib.awq_export_gptq(*ins, N, K, gs, bits, sym, off, *outs, None), _hip.last_error()

    def imp(N, K, gs, bits=4, sym=0, off=1, ins=(one, one, one), outs=(one, one, one, one)):
        return lib.awq_import_gptq(*ins, N, K, gs, bits, sym, off, *outs[:3], None), _hip.last_error()
    return lib, one, (export, imp)


def test_refusals_in_their_documented_order():
    lib, one, calls = _calls()
    none3, none4 = (None, None, None), (None, None, None, None)
    for call in calls:
        # each rule on its own
        assert call(-8, 64, 32)[0] == EINVAL and "negative" in call(-8, 64, 32)[1]
        assert call(8, -64, 32)[0] == EINVAL
        rc, msg = call(8, 64, 32, bits=8)
        assert rc == EUNSUPPORTED and "4-bit" in msg
        rc, msg = call(8, 64, 0)
        assert rc == EINVAL and "Group size" in msg
        for N, K, gs in ((12, 64, 32), (8, 36, 36), (8, 64, 48)):
            rc, msg = call(N, K, gs)
            assert rc == EINVAL and "% 8" in msg and "group_size" in msg, (N, K, gs)
        for off in (-1, 2):
            rc, msg = call(8, 64, 32, off=off)
            assert rc == EINVAL and "zero_offset" in msg
        rc, msg = call(8, 64, 32, sym=2)
        assert rc == EINVAL and "symmetric" in msg
        # an empty weight: AWQ_OK before any pointer is looked at
        assert call(0, 64, 32, ins=none3, outs=none4)[0] == OK
        assert call(8, 0, 32, ins=none3, outs=none4)[0] == OK
        # the AutoAWQ export's size limit, then N K
        rc, msg = call(8, 65536 * 256, 128)
        assert rc == EUNSUPPORTED and "65535" in msg
        assert call(65536 * 256, 64, 32)[0] == EUNSUPPORTED
        assert call(1 << 22, (1 << 20) + 512, 128)[0] == EUNSUPPORTED
        # pointers last
        rc, msg = call(8, 64, 32, outs=none4)
        assert rc == EINVAL and "at least one output" in msg
        for i in range(3):
            ins = tuple(None if j == i else one for j in range(3))
            rc, msg = call(8, 64, 32, ins=ins)
            assert rc == EINVAL and "without its input" in msg
        # the order: each earlier rule wins over every later one
        assert "negative" in call(-8, 36, 0, bits=8, off=5, outs=none4)[1]
        assert "4-bit" in call(12, 36, 0, bits=8, off=5, outs=none4)[1]
        assert "Group size" in call(12, 36, 0, off=5, outs=none4)[1]
        assert "% 8" in call(12, 64, 32, off=5, outs=none4)[1]
        assert "zero_offset" in call(8, 64, 32, off=5, sym=3, outs=none4)[1]
        assert "symmetric" in call(0, 64, 32, sym=3, outs=none4)[1]
        assert call(0, 65536 * 256, 128, ins=none3, outs=none4)[0] == OK
        assert "65535" in call(8, 65536 * 256, 128, outs=none4)[1]
    assert lib.awq_abi_version() == 17                               # additive


def test_api_shape_and_format_errors():
    from awq_quantizer.quantization import AWQQuantizer
    q = AWQQuantizer(bits=4, group_size=128, symmetric=False, device="cpu", logger_level="ERROR")
    ok = {"qweight": torch.zeros((32, 64), dtype=torch.int32), "qzeros": torch.zeros((2, 8), dtype=torch.int32),
          "scales": torch.zeros((2, 64), dtype=torch.float16)}
    for key, bad in (("qweight", torch.zeros((32, 60), dtype=torch.int32)),
                     ("qzeros", torch.zeros((3, 8), dtype=torch.int32)),
                     ("scales", torch.zeros((2, 72), dtype=torch.float16)),
                     ("scales", torch.zeros(128, dtype=torch.float16))):
        with pytest.raises(ValueError):
            q.import_gptq(dict(ok, **{key: bad}))
    with pytest.raises(ValueError, match="group_size"):
        q.import_gptq(ok, group_size=96)
    with pytest.raises(ValueError, match="checkpoint_format"):
        q.import_gptq(ok, checkpoint_format="marlin")
    with pytest.raises(ValueError, match="act-order"):
        q.import_gptq(dict(ok, g_idx=torch.zeros(256, dtype=torch.int32)))
    with pytest.raises(ValueError, match="checkpoint_format"):
        q.export_gptq({}, checkpoint_format="v3")


# ---------------------------------------------------------------- the flag rules
BASE = ["--model_id", "m", "--output_dir", "o"]
AWQ = ["--scale_method", "awq"]
STATS = AWQ + ["--act_stats", "s.safetensors"]
GPTQ = ["--output_format", "gptq"]
E_FOLD_NEEDS = "--fold_scales needs --scale_method awq, --act_stats and --output_format autoawq"
E_GPTQ_BITS = "--output_format gptq writes 4-bit checkpoints (AutoGPTQ layout, desc_act false)"
E_GPTQ_WORLD = "--output_format gptq runs in one process (it is not written under torchrun)"
E_STATS_GPTQ = ("--act_stats with --output_format gptq: the searched input scales must be folded "
                "into the ops producing each input first; use --output_format packed or reference "
                "(results carry 'input_scale'), or add --fold_scales")
CASES = [
    ("gptq", GPTQ, 1, 1, "opt", None),
    ("gptq symmetric v2", GPTQ + ["--symmetric", "--gptq_format", "gptq_v2"], 1, 2, None, None),
    ("gptq with --fold_scales", STATS + GPTQ + ["--fold_scales"], 1, 1, "llama", None),
    ("gptq with --fold_scales, symmetric, clipped", STATS + GPTQ + ["--fold_scales", "--symmetric", "--act_clip"], 1, 1,
     "qwen2", None),
    ("gptq at 8 bits", GPTQ + ["--bits", "8"], 1, 1, "llama", E_GPTQ_BITS),
    ("gptq under torchrun", GPTQ, 2, 1, "llama", E_GPTQ_WORLD),
    ("statistics to gptq, unfolded", STATS + GPTQ, 1, 1, "llama", E_STATS_GPTQ),
    ("fold to gptq without statistics", AWQ + GPTQ + ["--fold_scales"], 1, 1, "llama", E_FOLD_NEEDS),
    ("fold to gptq, unknown model type", STATS + GPTQ + ["--fold_scales"], 1, 1, "opt",
     "--fold_scales knows the block layout of model types llama, mistral, qwen2; config.json says 'opt'"),
    ("8-bit gptq beats unfolded statistics", STATS + GPTQ + ["--bits", "8"], 1, 1, "llama", E_GPTQ_BITS),
    ("--gptq_format alone changes nothing", ["--gptq_format", "gptq_v2"], 1, 1, None, None),
]


@pytest.mark.parametrize("label,argv,world,n_devices,model_type,expected", CASES, ids=[c[0] for c in CASES])
def test_check_args(label, argv, world, n_devices, model_type, expected):
    from awq_quantizer.options import check_args, parse_args
    assert check_args(parse_args(BASE + argv), world, n_devices, model_type) == expected


def test_gptq_format_choices():
    from awq_quantizer.options import parse_args
    assert parse_args(BASE + GPTQ).gptq_format == "gptq"
    with pytest.raises(SystemExit):
        parse_args(BASE + GPTQ + ["--gptq_format", "marlin"])


# ---------------------------------------------------------------- the writer and verify
GS = 32


def source_tensors():
    g = torch.Generator().manual_seed(3)
    mk = lambda *sh: (torch.randn(*sh, generator=g) * 0.05).bfloat16()
    return {"model.embed_tokens.weight": mk(64, 128), "model.norm.weight": torch.ones(128).bfloat16(),
            "model.layers.0.self_attn.q_proj.weight": mk(128, 128), "model.layers.0.mlp.down_proj.weight": mk(128, 160),
            "model.layers.0.mlp.down_proj.bias": mk(128), "lm_head.weight": mk(64, 128)}


def cpu_results(tensors, sym, fmt):
    """name -> what export_gptq returns, from the oracle's quantize and the helper's pack."""
    out = {}
    qmin = orc.qrange(4, sym)[0]
    for name, w in tensors.items():
        if not name.endswith("_proj.weight"):
            continue
        ref = orc.quantize(w, bits=4, group_size=GS, symmetric=sym)
        u, z = ref["tensor_q"].to(torch.int64) - qmin, ref["zero_points"].to(torch.int64) - qmin
        if not sym:
            u[0, :GS], z[0, 0] = (u[0, :GS] - z[0, 0]).clamp(0, 15), 0     # a zero point of 0 in every linear
        r = gl.pack(u, z, ref["scales"], GS, gl.ZERO_OFFSET[fmt])
        r["zero_points_at_0"] = torch.tensor(int((z == 0).sum()) if fmt == "gptq" else 0)
        out[name] = r
    return out


def write_dirs(tmp_path, sym=False, fmt="gptq", logger=None):
    from awq_quantizer.model_loading.safetensors_loader import SafetensorsLoader
    from awq_quantizer.options import parse_args
    from awq_quantizer.output import save_autoawq
    src, out = tmp_path / "src", tmp_path / "out"
    src.mkdir()
    out.mkdir()
    tensors = source_tensors()
    save_file(tensors, str(src / "model.safetensors"))
    with open(src / "config.json", "w") as f:
        json.dump({"model_type": "llama", "hidden_size": 128}, f)
    loader = SafetensorsLoader(model_path=str(src), logger_level="ERROR")
    results = cpu_results(tensors, sym, fmt)
    args = parse_args(["--model_id", str(src), "--output_dir", str(out), "--group_size", str(GS), "--output_format",
                       "gptq", "--gptq_format", fmt] + (["--symmetric"] if sym else []))
    save_autoawq(results, loader, [i for i in loader.tensor_index() if i.name not in results], str(out), args, logger)
    loader.close()
    return str(src), str(out), tensors, results


def cpu_import(gptq, group_size, symmetric, fmt):
    w = gl.to_packed_words(gptq, gl.ZERO_OFFSET[fmt])
    K8, N = gptq["qweight"].shape
    return dict(w, bits=torch.tensor(4, dtype=torch.int32), group_size=torch.tensor(group_size, dtype=torch.int32),
                symmetric=torch.tensor(symmetric, dtype=torch.bool), shape=torch.tensor([N, K8 * 8], dtype=torch.int64))


def run_verify(src, out, seen=None):
    from awq_quantizer import verify
    from awq_quantizer.quantization.awq import error_report

    def stub(tensor, result):
        if seen is not None:
            seen.append((tensor, result))
        n = tensor.numel()
        return error_report(n, [n * 0.5, n * 0.25, n * 4.0, 0.75, 0.0])

    args = verify.parse_args(["--model_id", src, "--quantized_dir", out, "--log_level", "CRITICAL"])
    rc = verify.verify(args, error_fn=stub, import_fn=cpu_import, fold_fn=lambda w, s: w)
    return rc, json.load(open(f"{out}/quantization_error.json"))


def rewrite(path, change):
    t = load_file(path)
    change(t)
    save_file(t, path)


class _Log:
    def __init__(self):
        self.warnings, self.infos = [], []

    def warning(self, m):
        self.warnings.append(m)

    def info(self, m):
        self.infos.append(m)


@pytest.mark.parametrize("sym,fmt", [(False, "gptq"), (False, "gptq_v2"), (True, "gptq")])
def test_writer_files_and_metadata(tmp_path, sym, fmt):
    log = _Log()
    src, out, tensors, results = write_dirs(tmp_path, sym, fmt, log)
    ck = load_file(out + "/model.safetensors")
    linears = [n[: -len(".weight")] for n in results]
    assert len(linears) == 2
    for l in linears:
        for f in ("qweight", "qzeros", "scales", "g_idx"):
            assert torch.equal(ck[f"{l}.{f}"].view(torch.int16) if f == "scales" else ck[f"{l}.{f}"],
                               results[l + ".weight"][f].view(torch.int16) if f == "scales" else results[l + ".weight"][f])
        assert f"{l}.weight" not in ck and f"{l}.zero_points_at_0" not in ck
    copied = set(tensors) - set(results)
    assert set(ck) == copied | {f"{l}.{f}" for l in linears for f in ("qweight", "qzeros", "scales", "g_idx")}
    for n in copied:
        assert torch.equal(ck[n].view(torch.int16), tensors[n].view(torch.int16))
    qc = json.load(open(out + "/quantize_config.json"))
    want = {"quant_method": "gptq", "bits": 4, "group_size": GS, "sym": sym, "desc_act": False, "checkpoint_format": fmt}
    assert {k: qc[k] for k in want} == want
    cfg = json.load(open(out + "/config.json"))
    assert cfg["quantization_config"] == want and cfg["model_type"] == "llama" and cfg["hidden_size"] == 128
    # zero points of 0: counted per tensor, warned about and recorded, under v1 only; never symmetric
    counts = {l: int(results[l + ".weight"]["zero_points_at_0"]) for l in linears}
    if fmt == "gptq" and not sym:
        assert all(c >= 1 for c in counts.values())
        assert qc["meta"] == {"zero_points_at_0": sum(counts.values()), "zero_points_at_0_per_tensor": counts}
        assert len(log.warnings) == 2 and all(str(counts[l]) in w and l in w for l, w in zip(linears, log.warnings))
    else:
        assert qc["meta"] == {"zero_points_at_0": 0, "zero_points_at_0_per_tensor": {}} and log.warnings == []
    assert any("Saved GPTQ checkpoint" in m for m in log.infos)


@pytest.mark.parametrize("sym,fmt", [(False, "gptq"), (True, "gptq_v2")])
def test_clean_directory_verifies(tmp_path, sym, fmt):
    from awq_quantizer import verify
    from awq_quantizer.evaluation.checkpoint import QuantizedCheckpoint
    src, out, tensors, results = write_dirs(tmp_path, sym, fmt)
    assert verify.is_gptq_dir(out) and verify.is_autoawq_dir(out) and not verify.is_gptq_dir(src)
    assert verify.read_gptq_config(out) == ({"group_size": GS, "symmetric": sym, "checkpoint_format": fmt,
                                             "not_converted": []}, {})
    seen = []
    rc, rep = run_verify(src, out, seen)
    assert rc == 0 and rep["problems"] == {} and rep["layout"] == "gptq" and rep["fold_audited"] is False
    assert set(rep["tensors"]) == set(results) and all(e["layout"] == "gptq" for e in rep["tensors"].values())
    assert set(rep["copied"]) == set(tensors) - set(results)         # g_idx is part of its linear, not a copy
    for tensor, result in seen:                                      # the imported words are the row-major ones
        assert bool(result["symmetric"]) == sym and int(result["group_size"]) == GS
    # evaluate's loader: every linear through the gptq dequantizer, with the directory's settings
    calls = []

    class Stub:
        def gptq(self, gptq, gs, s, f):
            calls.append((gs, s, f, sorted(gptq)))
            return gl.dequantize(gptq, gl.ZERO_OFFSET[f])

    from awq_quantizer.model_loading.safetensors_loader import SafetensorsLoader
    loader = SafetensorsLoader(model_path=src, logger_level="ERROR")
    ck = QuantizedCheckpoint(loader, out, Stub())
    assert ck.format == "gptq" and ck.quantized_names() == sorted(results)
    for info in loader.tensor_index():
        w = ck.read(info)
        if info.name in results:
            assert torch.equal(w, gl.dequantize(results[info.name], gl.ZERO_OFFSET[fmt]))
        else:
            assert torch.equal(w.view(torch.int16), tensors[info.name].view(torch.int16))
    assert calls == [(GS, sym, fmt, ["g_idx", "qweight", "qzeros", "scales"])] * 2
    ck.close()
    loader.close()


def test_verify_reports_an_act_order_g_idx(tmp_path):
    src, out, _, _ = write_dirs(tmp_path)
    key = "model.layers.0.mlp.down_proj.g_idx"

    def alter(t):
        t[key] = t[key].clone()
        t[key][37] = 0                                               # one entry: 37 // 32 = 1
    rewrite(out + "/model.safetensors", alter)
    rc, rep = run_verify(src, out)
    name = "model.layers.0.mlp.down_proj.weight"
    assert rc == 1 and set(rep["problems"]) == {name}
    assert "g_idx[37]" in rep["problems"][name] and "act-order" in rep["problems"][name]
    assert "not supported" in rep["problems"][name]
    assert set(rep["tensors"]) == {"model.layers.0.self_attn.q_proj.weight"}


@pytest.mark.parametrize("fmt", ["gptq", "gptq_v2"])
def test_verify_reports_a_symmetric_zero_other_than_8(tmp_path, fmt):
    src, out, _, _ = write_dirs(tmp_path, sym=True, fmt=fmt)
    rc, rep = run_verify(src, out)
    assert rc == 0
    key = "model.layers.0.self_attn.q_proj.qzeros"

    def alter(t):
        t[key] = t[key].clone()
        t[key][2, 5] ^= 1 << 12                                      # one nibble of one word
    rewrite(out + "/model.safetensors", alter)
    rc, rep = run_verify(src, out)
    name = "model.layers.0.self_attn.q_proj.weight"
    assert rc == 1 and set(rep["problems"]) == {name} and "other than 8" in rep["problems"][name]


@pytest.mark.parametrize("value", [None, "marlin"])
def test_verify_reports_a_missing_or_unknown_checkpoint_format(tmp_path, value):
    src, out, _, _ = write_dirs(tmp_path)
    for fname, key in (("quantize_config.json", None), ("config.json", "quantization_config")):
        cfg = json.load(open(f"{out}/{fname}"))
        d = cfg[key] if key else cfg
        if value is None:
            del d["checkpoint_format"]
        else:
            d["checkpoint_format"] = value
        json.dump(cfg, open(f"{out}/{fname}", "w"))
    rc, rep = run_verify(src, out)
    assert rc == 1 and set(rep["problems"]) == {"quantize_config.json"} and rep["tensors"] == {}
    assert "checkpoint_format" in rep["problems"]["quantize_config.json"]
    assert "missing or unknown" in rep["problems"]["quantize_config.json"] and rep["layout"] == "gptq"
