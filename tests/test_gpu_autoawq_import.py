"""awq_import_autoawq_gemm (csrc/awq_import.hip), AWQQuantizer.import_autoawq / dequantize_autoawq
and verify on AutoAWQ directories, on the GPU.

The CPU restatement is the oracle's: autoawq_pack / autoawq_unpack for the GEMM layout, pack_rows
for the row-major one.  Shapes are the smallest that reach each path of the kernels: one partial
tile; G = 3 (padding nibbles of qzeros); ragged in both qweight tile edges with N/8 % 4 != 0 (4-B
loads); gs 64; gs 8 with K/8 % 4 != 0 (4-B stores) and G % 8 != 0 (scalar group kernel); N % 32 == 0
with several k tiles (16-B loads and stores).  Each shape's reference is computed once."""
import json
import math
import os

import pytest
import torch
from safetensors.torch import load_file, save_file

from oracle import awq_oracle as orc
from test_gpu_bounds import Call, _dev, _lib, _stream

pytestmark = pytest.mark.gpu

SHAPES = [(8, 128, 128), (72, 384, 128), (296, 2304, 128), (776, 512, 64), (24, 264, 8), (40, 2072, 8),
          (520, 8192, 128)]
_ids = lambda v: str(v).replace("torch.", "")
_REF = {}


def quantizer(gs, sym=False):
    from awq_quantizer.quantization import AWQQuantizer
    return AWQQuantizer(bits=4, group_size=gs, symmetric=sym, device="cuda:0", logger_level="ERROR")


def bits16(t):
    return t.cpu().contiguous().view(torch.int16)


def reference(N, K, gs, words):
    """(GEMM-layout inputs, row-major expectation) of a shape: from random fields through
    autoawq_pack, or (words) from random 32-bit words through autoawq_unpack; shared by the tests."""
    key = (N, K, gs, words)
    if key not in _REF:
        G = K // gs
        g = torch.Generator().manual_seed(N * 7 + K + gs + int(words))
        sc = torch.randint(-2 ** 15, 2 ** 15, (N, G), generator=g, dtype=torch.int16).view(torch.float16)
        if words:
            qw_t = torch.randint(-2 ** 31, 2 ** 31, (K, N // 8), generator=g, dtype=torch.int64).to(torch.int32)
            qz_t = torch.randint(-2 ** 31, 2 ** 31, (G, N // 8), generator=g, dtype=torch.int64).to(torch.int32)
            f, z = orc.autoawq_unpack(qw_t, qz_t)
            f, z = f.t().contiguous(), z.t().contiguous()
        else:
            f = torch.randint(0, 16, (N, K), generator=g)
            z = torch.randint(0, 16, (N, G), generator=g)
            qw_t, qz_t, _ = orc.autoawq_pack(f, z, sc)
        gemm = {"qweight": qw_t, "qzeros": qz_t, "scales": sc.t().contiguous()}
        want = {"qweight": orc.pack_rows(f.to(torch.int32), 4, 0), "qzeros": orc.pack_rows(z.to(torch.int32), 4, 0),
                "scales": sc}
        assert want["qzeros"].shape == (N, -(-G // 8))
        _REF[key] = (gemm, want)
    return _REF[key]


# ---------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("words", [False, True], ids=["fields", "words"])
@pytest.mark.parametrize("N,K,gs", SHAPES, ids=_ids)
def test_import_matches_the_oracle(N, K, gs, words):
    _dev()
    gemm, want = reference(N, K, gs, words)
    got = quantizer(gs).import_autoawq(gemm)
    assert got["qweight"].is_cuda and tuple(got["shape"].tolist()) == (N, K)
    assert int(got["bits"]) == 4 and int(got["group_size"]) == gs and not bool(got["symmetric"])
    assert torch.equal(got["qweight"].cpu(), want["qweight"])
    assert torch.equal(got["qzeros"].cpu(), want["qzeros"])              # pad fields of the last word are 0
    assert torch.equal(bits16(got["scales"]), bits16(want["scales"]))
    back = quantizer(gs).export_autoawq(got)                              # and the export takes the result
    assert torch.equal(back["qweight"].cpu(), gemm["qweight"])
    assert torch.equal(back["qzeros"].cpu(), gemm["qzeros"])
    assert torch.equal(bits16(back["scales"]), bits16(gemm["scales"]))


@pytest.mark.parametrize("which", ["scales", "qweight", "qzeros"])
@pytest.mark.parametrize("N,K,gs", [(72, 384, 128), (296, 2304, 128)], ids=_ids)
def test_selective_outputs(N, K, gs, which):
    """One output only: the others are NULL, and so are their inputs (they are not looked at)."""
    dev = _dev()
    from awq_quantizer import _hip
    gemm, want = reference(N, K, gs, True)
    src = gemm[which].to(dev)
    out = torch.empty_like(want[which], device=dev)
    args = {k: (src if k == which else None) for k in ("qweight", "qzeros", "scales")}
    outs = {k: (out if k == which else None) for k in ("qweight", "qzeros", "scales")}
    _hip.import_autoawq_gemm(args["qweight"], args["qzeros"], args["scales"], N, K, gs, 4, outs["qweight"],
                             outs["qzeros"], outs["scales"])
    view = bits16 if which == "scales" else (lambda t: t.cpu())
    assert torch.equal(view(out), view(want[which]))


# ---------------------------------------------------------------- round trip and dequantize
@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=_ids)
@pytest.mark.parametrize("N,K,gs", SHAPES, ids=_ids)
def test_round_trip_is_word_for_word(N, K, gs, dtype, sym):
    """import(export(p)) == p for p = quantize_packed(x); G % 8 != 0 pins the padding rule."""
    _dev()
    g = torch.Generator().manual_seed(N + K)
    x = (torch.randn(N, K, generator=g) * 0.02).to(dtype)
    q = quantizer(gs, sym)
    p = q.quantize_packed(x)
    r = q.import_autoawq(q.export_autoawq(p))
    for k in ("qweight", "qzeros"):
        assert torch.equal(r[k], p[k]), k
    assert torch.equal(r["scales"].view(torch.int16), p["scales"].view(torch.int16))
    for k in ("bits", "group_size", "symmetric", "shape"):
        assert torch.equal(r[k], p[k]) and r[k].dtype == p[k].dtype, k


@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
@pytest.mark.parametrize("N,K,gs", [(72, 384, 128), (296, 2304, 128), (24, 264, 8)], ids=_ids)
def test_dequantize_autoawq_equals_the_reference(N, K, gs, sym):
    _dev()
    g = torch.Generator().manual_seed(N + K + 1)
    x = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    q = quantizer(gs, sym)
    ref = orc.quantize(x, bits=4, group_size=gs, symmetric=sym)
    dq = q.dequantize_autoawq(q.export_autoawq(q.quantize_packed(x)))
    assert dq.shape == (N, K) and dq.dtype == torch.float32
    assert torch.equal(dq.cpu().view(torch.int32), orc.dequantize(ref).view(torch.int32))


def test_import_refuses_on_the_device():
    _dev()
    gemm, _ = reference(72, 384, 128, False)
    with pytest.raises(ValueError, match="qzeros"):
        quantizer(64).import_autoawq(gemm)
    with pytest.raises(ValueError, match="group_size"):
        quantizer(256).import_autoawq(gemm)


# ---------------------------------------------------------------- the nontemporal path
def _torch_row_major(qweight_t, qzeros_t, scales_t, N, K, G):
    """The row-major layout of GEMM-layout words, restated with torch tensor ops on the device
    (unpack nibbles, undo AWQ_ORDER, transpose, repack; pad fields 0)."""
    dev = qweight_t.device
    rev = torch.tensor(orc.AWQ_REVERSE_ORDER, device=dev)
    sh = 4 * torch.arange(8, device=dev, dtype=torch.int64)

    def unpack(w):                                  # [R, N / 8] words -> [R, N] fields, natural order
        return ((w.to(torch.int64).unsqueeze(-1) >> sh) & 15)[:, :, rev].reshape(w.shape[0], -1)

    def pack(v):                                    # [N, C] fields -> [N, ceil(C / 8)] words
        pad = (-v.shape[1]) % 8
        if pad:
            v = torch.nn.functional.pad(v, (0, pad))
        x = (v.reshape(v.shape[0], -1, 8) << sh).sum(-1)
        return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)

    return pack(unpack(qweight_t).t().contiguous()), pack(unpack(qzeros_t).t().contiguous()), scales_t.t().contiguous()


def test_large_nontemporal_path():
    """qweight outputs of >= 128 MB take the nontemporal-store kernel (AWQ_EXPORT_NT_MIN): random
    words against the torch restatement on the device (the export test's shape)."""
    dev = _dev()
    N, K, gs = 32768, 8192, 128
    G = K // gs
    assert N * K // 2 >= 128 << 20
    g = torch.Generator(device=dev).manual_seed(N + K)
    info = torch.iinfo(torch.int32)
    gemm = {"qweight": torch.randint(info.min, info.max, (K, N // 8), generator=g, device=dev, dtype=torch.int32),
            "qzeros": torch.randint(info.min, info.max, (G, N // 8), generator=g, device=dev, dtype=torch.int32),
            "scales": torch.randn(G, N, generator=g, device=dev).half()}
    got = quantizer(gs).import_autoawq(gemm)
    qw, qz, sc = _torch_row_major(gemm["qweight"], gemm["qzeros"], gemm["scales"], N, K, G)
    assert torch.equal(got["qweight"], qw)
    assert torch.equal(got["qzeros"], qz)
    assert torch.equal(got["scales"].view(torch.int16), sc.view(torch.int16))


# ---------------------------------------------------------------- guard bands
@pytest.mark.parametrize("outs", ["all", "scales", "qweight"])
@pytest.mark.parametrize("N,K,gs,skew", [(8, 128, 128, 0), (72, 512, 64, 0), (264, 288, 32, 0), (24, 264, 8, 0),
                                         (288, 2176, 128, 0), (288, 2176, 128, 4), (72, 512, 64, 4)], ids=_ids)
def test_guard_bands(N, K, gs, skew, outs):
    """Every path out of the guard-band arena, on dirty outputs, in both fill polarities: nothing
    outside the outputs changes and every output byte is the expectation's.  N % 32 == 0 and
    aligned: 16-B qweight loads, else 4-B; K/8 % 4 == 0 and aligned: 16-B stores, else 4-B; G % 8 == 0
    and aligned scales: the vector group kernel, else the scalar one; skew 4: every pointer 4-B but
    not 16-B aligned; 288 x 2176 is ragged in both qweight tile edges and has G = 17."""
    dev = _dev()
    G = K // gs
    assert N % 8 == 0 and K % gs == 0
    assert (N % 32 == 0) == (N == 288) and ((K // 8) % 4 == 0) == (K != 264) and (G % 8 == 0) == (K == 512)
    gemm, want = reference(N, K, gs, True)
    c = Call(dev, seed=N + K + skew)
    use = ("qweight", "qzeros", "scales") if outs == "all" else (outs,)
    ib = {k: c.inp(k + "_t", gemm[k], skew=skew) for k in use}
    ob = {k: c.out(k, want[k], skew=skew) for k in use}
    c.build()
    assert all(b.addr % 16 == skew for b in list(ib.values()) + list(ob.values()))
    p = lambda d, k: d[k].ptr if k in d else None
    c.run(lambda: _lib().awq_import_autoawq_gemm(p(ib, "qweight"), p(ib, "qzeros"), p(ib, "scales"), N, K, gs, 4,
                                                 p(ob, "qweight"), p(ob, "qzeros"), p(ob, "scales"), _stream(dev)))


# ---------------------------------------------------------------- verify, end to end
L = "model.layers"


def _block(prefix, g):
    mk = lambda *sh: (torch.randn(*sh, generator=g) * 0.05).bfloat16()
    t = {f"{prefix}.input_layernorm.weight": (1 + 0.1 * torch.randn(128, generator=g)).bfloat16(),
         f"{prefix}.post_attention_layernorm.weight": (1 + 0.1 * torch.randn(128, generator=g)).bfloat16()}
    for n in "qkvo":
        t[f"{prefix}.self_attn.{n}_proj.weight"] = mk(128, 128)
    t[f"{prefix}.self_attn.v_proj.bias"] = mk(128)
    t.update({f"{prefix}.mlp.gate_proj.weight": mk(256, 128), f"{prefix}.mlp.up_proj.weight": mk(256, 128),
              f"{prefix}.mlp.down_proj.weight": mk(128, 256)})
    return t


def _stats(prefix, g, tokens=64):
    def st(K, hot):
        x = torch.randn(tokens, K, generator=g)
        x[:, hot] *= 30
        return x.abs().mean(0), (x * x).mean(0)
    a, o, m, d = st(128, 3), st(128, 17), st(128, 40), st(256, 99)
    out = {f"{prefix}.self_attn.{n}_proj.weight": a for n in "qkv"}
    out[f"{prefix}.self_attn.o_proj.weight"] = o
    out.update({f"{prefix}.mlp.gate_proj.weight": m, f"{prefix}.mlp.up_proj.weight": m,
                f"{prefix}.mlp.down_proj.weight": d})
    return out


@pytest.fixture(scope="module")
def tiny_llama(tmp_path_factory):
    """A 2-block Llama directory (hidden 128, MHA: attn_out and mlp_out both fold; v_proj has a
    bias) and the activation statistics of every linear."""
    d = tmp_path_factory.mktemp("tiny_llama_import")
    g = torch.Generator().manual_seed(77)
    tensors = {"model.embed_tokens.weight": torch.randn(256, 128, generator=g).bfloat16(),
               "model.norm.weight": torch.ones(128).bfloat16(),
               "lm_head.weight": torch.randn(256, 128, generator=g).bfloat16()}
    flat = {}
    for i in range(2):
        tensors.update(_block(f"{L}.{i}", g))
        for name, (xm, xs) in _stats(f"{L}.{i}", g).items():
            flat[name + ".x_mean"], flat[name + ".x_sq"] = xm.clone(), xs.clone()
    save_file(tensors, str(d / "model.safetensors"))
    with open(d / "config.json", "w") as f:
        json.dump({"model_type": "llama", "hidden_size": 128}, f)
    stats_path = str(tmp_path_factory.mktemp("tiny_llama_import_stats") / "stats.safetensors")
    save_file(flat, stats_path)
    return str(d), stats_path, tensors


def _by_hand(out, tensors):
    """quantization_error of every linear of the directory, called by hand on the rebuilt domain."""
    from awq_quantizer import _hip
    dev = torch.device("cuda", 0)
    q = quantizer(32)
    st = load_file(os.path.join(out, "model.safetensors"))
    side_path = os.path.join(out, "awq_scales.safetensors")
    side = load_file(side_path) if os.path.exists(side_path) else {}
    res = {}
    for key in st:
        if not key.endswith(".qweight"):
            continue
        layer = key[:-len(".qweight")]
        name = layer + ".weight"
        r = q.import_autoawq({k: st[f"{layer}.{k}"] for k in ("qweight", "qzeros", "scales")}, 32, False)
        w = tensors[name].to(dev)
        if f"{name}.row_scale" in side:
            w = _hip.fold_rows(w.contiguous(), side[f"{name}.row_scale"].to(dev))
        if f"{name}.input_scale" in side:
            r["input_scale"] = side[f"{name}.input_scale"]
        res[name] = q.quantization_error(w, r)
    return res


def _same_number(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("clip", [False, True], ids=["rtn", "act_clip"])
def test_verify_fold_scales_checkpoint(tiny_llama, tmp_path, clip):
    from awq_quantizer import verify
    from awq_quantizer.main import main
    _dev()
    d, p, tensors = tiny_llama
    out = str(tmp_path / "out")
    assert main(["--model_id", d, "--log_level", "ERROR", "--group_size", "32", "--device", "cuda:0", "--output_dir",
                 out, "--scale_method", "awq", "--act_stats", p, "--output_format", "autoawq", "--fold_scales"]
                + (["--act_clip"] if clip else [])) == 0
    vargs = ["--model_id", d, "--quantized_dir", out, "--log_level", "ERROR", "--device", "cuda:0"]
    assert verify.main(vargs) == 0
    rep = json.load(open(os.path.join(out, "quantization_error.json")))
    assert rep["problems"] == {} and rep["layout"] == "autoawq" and rep["fold_audited"] is True
    hand = _by_hand(out, tensors)
    assert set(rep["tensors"]) == set(hand) and len(hand) == 14
    for name, e in rep["tensors"].items():
        for k in ("numel", "nonfinite", "sum_abs", "sum_sq", "sum_w_sq", "mean_abs_error", "mse", "max_abs_error",
                  "snr_db"):
            assert _same_number(e[k], hand[name][k]), (name, k, e[k], hand[name][k])
        assert e["layout"] == "autoawq" and e["input_scaled"] is True
        assert e["row_folded"] == (name.endswith("v_proj.weight") or name.endswith("up_proj.weight")), name
        assert e["nonfinite"] == 0 and math.isfinite(e["snr_db"]), (name, e["snr_db"])
    assert set(rep["copied"]) == {n for n in tensors if n not in hand}
    # one norm put back to the source's: verify names it
    norm = f"{L}.1.post_attention_layernorm.weight"
    path = os.path.join(out, "model.safetensors")
    st = load_file(path)
    assert not torch.equal(st[norm], tensors[norm])
    st[norm] = tensors[norm].clone()
    save_file(st, path, metadata={"format": "pt"})
    assert verify.main(vargs) == 1
    rep = json.load(open(os.path.join(out, "quantization_error.json")))
    assert set(rep["problems"]) == {norm} and len(rep["tensors"]) == 14


def test_verify_plain_autoawq_directory(tiny_llama, tmp_path):
    from awq_quantizer import verify
    from awq_quantizer.main import main
    _dev()
    d, _, tensors = tiny_llama
    out = str(tmp_path / "plain")
    assert main(["--model_id", d, "--log_level", "ERROR", "--group_size", "32", "--device", "cuda:0", "--output_dir",
                 out, "--output_format", "autoawq"]) == 0
    assert not os.path.exists(os.path.join(out, "awq_scales.safetensors"))
    assert verify.main(["--model_id", d, "--quantized_dir", out, "--log_level", "ERROR", "--device", "cuda:0"]) == 0
    rep = json.load(open(os.path.join(out, "quantization_error.json")))
    hand = _by_hand(out, tensors)
    assert rep["problems"] == {} and rep["fold_audited"] is False and set(rep["tensors"]) == set(hand)
    for name, e in rep["tensors"].items():
        assert e["input_scaled"] is False and e["row_folded"] is False and e["layout"] == "autoawq"
        assert _same_number(e["sum_sq"], hand[name]["sum_sq"]) and _same_number(e["snr_db"], hand[name]["snr_db"])
