"""Scale folding on the GPU (include/awq_hip.h awq_fold_rows, AWQQuantizer.quantize_block,
--fold_scales):
  1. the kernel, bit for bit against torch's CPU result of (w.float() / s[:, None]).to(dtype);
  2. quantize_block against the same public calls made by hand in the documented order, the row
     fold done by that torch-CPU expression;
  3. the fold is an equivalence: a float64 forward of the block with the folded norms / biases
     and W' = W diag(input_scale) / row_scale equals the forward of the source;
  4. the CLI end to end."""
import json
import math
import os

import pytest
import torch
from safetensors.torch import load_file, save_file

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# the smallest shapes that reach each path and boundary of the kernel
SHAPES = {
    "fast_smallest": (1, 8),
    "fast_tile_spans_256_rows": (300, 8),
    "fast_rows_straddle_tiles": (3, 2056),
    "fast_partial_last_tile": (257, 136),
    "fast_row_aligned_tiles": (64, 2048),
    "element": (3, 5),
    "vector_K1": (129,),
    "element_offset_view": (16, 64),
}
L = "model.layers"
EXTRA = f"{L}.1.self_attn.extra_proj.weight"


def _dev():
    from awq_quantizer import _hip
    dev = torch.device("cuda", 0)
    _hip.require_device(dev)
    return dev


def cpu_fold(w: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """The oracle: an fp32 IEEE division, then one rounding into the dtype (torch CPU)."""
    w, s = w.cpu(), s.cpu().float()
    return (w.float() / s.reshape([-1] + [1] * (w.dim() - 1))).to(w.dtype)


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bit-equal, NaNs compared by position (payloads are unspecified)."""
    got, want = got.cpu(), want.cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    gn, wn = torch.isnan(got), torch.isnan(want)
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    return torch.equal(gn, wn) and torch.equal(got.view(it)[~gn], want.view(it)[~wn])


# ---------------------------------------------------------------- 1. the kernel
_CASES = {}


def fold_case(case: str, dtype):
    """(w, s, expectation) of a case, computed once and shared (never modified)."""
    key = (case, dtype)
    if key not in _CASES:
        shape = SHAPES[case]
        g = torch.Generator().manual_seed(10 * list(SHAPES).index(case) + DTYPES.index(dtype))
        w = torch.randn(shape, generator=g).to(dtype)
        flat = w.view(-1)
        n = flat.numel()
        tiny = torch.finfo(dtype).tiny     # smallest normal: tiny / 8 is a subnormal input with a subnormal
        specials = (float("inf"), 0.0, float("nan"), float("-inf"), tiny / 8, -1.5 * tiny)   # quotient for s > 1/8
        for i, v in enumerate(specials):   # spread over the tensor
            flat[(i * n) // len(specials) + (1 if n > 8 else 0)] = v
        s = torch.exp(torch.randn(shape[0], generator=g))
        _CASES[key] = (w, s, cpu_fold(w, s))
    return _CASES[key]


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("case", list(SHAPES))
def test_fold_rows_bit_exact(case, dtype, in_place):
    from awq_quantizer import _hip
    dev = _dev()
    w, s, want = fold_case(case, dtype)
    assert torch.isnan(want).any() and torch.isinf(want).any() and (want == 0).any()
    assert ((want.float().abs() < torch.finfo(dtype).tiny) & (want != 0)).any()      # a subnormal quotient
    if case == "element_offset_view":      # an aligned shape behind a storage offset of one element
        base = torch.zeros(w.numel() + 8, dtype=dtype, device=dev)
        wd = base[1:1 + w.numel()].view(w.shape)
        wd.copy_(w)
        assert wd.storage_offset() == 1 and wd.data_ptr() % 16 != 0 and wd.is_contiguous()
    else:
        wd = w.to(dev)
        assert wd.data_ptr() % 16 == 0
    sd = s.to(dev)
    if in_place:
        got = _hip.fold_rows(wd, sd, out=wd)
        assert got.data_ptr() == wd.data_ptr()
    else:
        got = _hip.fold_rows(wd, sd)
        assert got.data_ptr() != wd.data_ptr() and same_bits(wd, w)      # the source is untouched
    assert same_bits(got, want)
    if case == "element_offset_view":      # nothing written outside the view
        assert float(base[0]) == 0 and not base[1 + w.numel():].any()


# ---------------------------------------------------------------- 2. / 3. / 4.: blocks
def block_tensors(prefix, hidden, inter, kv, dtype, seed, bias=False):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *sh: (torch.randn(*sh, generator=g) * 0.05).to(dtype)
    t = {f"{prefix}.input_layernorm.weight": (1 + 0.1 * torch.randn(hidden, generator=g)).to(dtype),
         f"{prefix}.post_attention_layernorm.weight": (1 + 0.1 * torch.randn(hidden, generator=g)).to(dtype),
         f"{prefix}.self_attn.q_proj.weight": mk(hidden, hidden), f"{prefix}.self_attn.k_proj.weight": mk(kv, hidden),
         f"{prefix}.self_attn.v_proj.weight": mk(kv, hidden), f"{prefix}.self_attn.o_proj.weight": mk(hidden, hidden),
         f"{prefix}.mlp.gate_proj.weight": mk(inter, hidden), f"{prefix}.mlp.up_proj.weight": mk(inter, hidden),
         f"{prefix}.mlp.down_proj.weight": mk(hidden, inter)}
    if bias:
        t.update({f"{prefix}.self_attn.q_proj.bias": mk(hidden), f"{prefix}.self_attn.k_proj.bias": mk(kv),
                  f"{prefix}.self_attn.v_proj.bias": mk(kv)})
    return t


def block_stats(prefix, hidden, inter, seed, tokens=64):
    """Statistics of a random x [tokens, in] with one 30x outlier channel, per input; linears
    reading one input share them."""
    g = torch.Generator().manual_seed(seed)

    def st(K, hot):
        x = torch.randn(tokens, K, generator=g)
        x[:, hot] *= 30
        return x.abs().mean(0), (x * x).mean(0)

    a, o, m, d = st(hidden, 3), st(hidden, 17), st(hidden, 40), st(inter, 99)
    out = {f"{prefix}.self_attn.{n}_proj.weight": a for n in "qkv"}
    out[f"{prefix}.self_attn.o_proj.weight"] = o
    out.update({f"{prefix}.mlp.gate_proj.weight": m, f"{prefix}.mlp.up_proj.weight": m,
                f"{prefix}.mlp.down_proj.weight": d})
    return out


def quantizer(gs=32):
    from awq_quantizer.quantization import AWQQuantizer
    return AWQQuantizer(bits=4, group_size=gs, symmetric=False, scale_method="awq", device="cuda:0",
                        logger_level="ERROR")


def plan_of(tensors, model_type="llama", gs=32):
    from awq_quantizer.quantization.block_plan import plan_blocks
    return plan_blocks({n: tuple(t.shape) for n, t in tensors.items()}, model_type, gs)


def same_result(a, b) -> bool:
    return all(torch.equal(a[f].cpu(), b[f].cpu()) for f in ("qweight", "qzeros", "scales")) and \
        torch.equal(a["shape"], b["shape"])


@pytest.mark.parametrize("clip", [False, True], ids=["rtn", "clip"])
@pytest.mark.parametrize("kv", [128, 64], ids=["mha", "gqa"])
def test_quantize_block_equals_the_calls_by_hand(kv, clip):
    dev = _dev()
    p = f"{L}.0"
    T = block_tensors(p, 128, 256, kv, torch.bfloat16, seed=kv)
    S = block_stats(p, 128, 256, seed=5)
    (block,) = plan_of(T)
    q = quantizer()
    ckw = {"clip": True, "clip_grid": 20, "clip_max_shrink": 0.5} if clip else {}
    out = q.quantize_block(T, S, block, **ckw)
    n = lambda m: f"{p}.{m}.weight"
    assert set(out["results"]) == set(block.members())
    assert all("input_scale" not in r for r in out["results"].values())

    def group(weights, ref):
        return q.quantize_layer_group({k: v.to(dev) for k, v in weights.items()}, x_mean=S[ref][0], x_sq=S[ref][1],
                                      **ckw)

    # 1. the output groups, 2. their row folds (torch CPU), 3. the input groups on the folded producers
    want, v_in = {}, T[n("self_attn.v_proj")]
    if kv == 128:
        ro = group({n("self_attn.o_proj"): T[n("self_attn.o_proj")]}, n("self_attn.o_proj"))
        want.update(ro["results"])
        v_in = cpu_fold(v_in, ro["input_scale"])
        assert torch.equal(out["scales"][n("self_attn.v_proj") + ".row_scale"].cpu(), ro["input_scale"].cpu())
        assert out["groups"]["attn_out"]["folded"] and out["groups"]["attn_out"]["ratio"] == ro["ratio"]
    else:
        o = T[n("self_attn.o_proj")].to(dev)
        if clip:
            ones = torch.ones((q.search_grid, 128), dtype=torch.float32, device=dev)
            so = S[n("self_attn.o_proj")]
            want[n("self_attn.o_proj")] = q.quantize_layer_group(
                {"o": o}, x_mean=so[0], x_sq=so[1], table=ones, **ckw)["results"]["o"]
        else:
            want[n("self_attn.o_proj")] = q.quantize_packed(o)
        assert n("self_attn.v_proj") + ".row_scale" not in out["scales"]
        assert not out["groups"]["attn_out"]["folded"]
        assert torch.equal(out["scales"][n("self_attn.o_proj") + ".input_scale"].cpu(), torch.ones(128))
    rd = group({n("mlp.down_proj"): T[n("mlp.down_proj")]}, n("mlp.down_proj"))
    want.update(rd["results"])
    up_in = cpu_fold(T[n("mlp.up_proj")], rd["input_scale"])
    assert torch.equal(out["scales"][n("mlp.up_proj") + ".row_scale"].cpu(), rd["input_scale"].cpu())
    ra = group({n("self_attn.q_proj"): T[n("self_attn.q_proj")], n("self_attn.k_proj"): T[n("self_attn.k_proj")],
                n("self_attn.v_proj"): v_in}, n("self_attn.q_proj"))
    rm = group({n("mlp.gate_proj"): T[n("mlp.gate_proj")], n("mlp.up_proj"): up_in}, n("mlp.gate_proj"))
    want.update(ra["results"])
    want.update(rm["results"])
    for name in block.members():
        assert same_result(out["results"][name], want[name]), name
    if clip:
        assert out["groups"]["attn_in"]["clip"]["loss_after"] <= out["groups"]["attn_in"]["clip"]["loss_before"]
    # every member's scale is reported
    for r in (ra, rm):
        for name in r["results"]:
            assert torch.equal(out["scales"][name + ".input_scale"].cpu(), r["input_scale"].cpu()), name
    assert set(out["scales"]) == {m + ".input_scale" for m in block.members()} | {
        k for k in (n("self_attn.v_proj") + ".row_scale", n("mlp.up_proj") + ".row_scale")
        if kv == 128 or "up_proj" in k}
    # 4. the norm folds
    assert set(out["folded"]) == {f"{p}.input_layernorm.weight", f"{p}.post_attention_layernorm.weight"}
    assert same_bits(out["folded"][f"{p}.input_layernorm.weight"],
                     cpu_fold(T[f"{p}.input_layernorm.weight"], out["scales"][n("self_attn.q_proj") + ".input_scale"]))
    assert same_bits(out["folded"][f"{p}.post_attention_layernorm.weight"],
                     cpu_fold(T[f"{p}.post_attention_layernorm.weight"],
                              out["scales"][n("mlp.gate_proj") + ".input_scale"]))
    assert not torch.equal(ra["input_scale"].cpu(), torch.ones(128))


def forward64(x, T, p, heads, eps=1e-6):
    """float64 CPU forward of one block: RMSNorm, causal softmax attention without RoPE, SwiGLU,
    both residuals.  T: name -> float64 tensor."""
    def norm(h, w):
        return h / torch.sqrt((h * h).mean(-1, keepdim=True) + eps) * w

    def lin(h, mod):
        y = h @ T[f"{p}.{mod}.weight"].T
        b = T.get(f"{p}.{mod}.bias")
        return y if b is None else y + b

    n, hid = x.shape
    h = norm(x, T[f"{p}.input_layernorm.weight"])
    q, k, v = (lin(h, f"self_attn.{m}_proj").reshape(n, heads, hid // heads).transpose(0, 1) for m in "qkv")
    att = q @ k.transpose(1, 2) / math.sqrt(hid // heads)
    att = att.masked_fill(torch.triu(torch.ones(n, n, dtype=torch.bool), 1), float("-inf")).softmax(-1)
    x = x + lin((att @ v).transpose(0, 1).reshape(n, hid), "self_attn.o_proj")
    h = norm(x, T[f"{p}.post_attention_layernorm.weight"])
    return x + lin(torch.nn.functional.silu(lin(h, "mlp.gate_proj")) * lin(h, "mlp.up_proj"), "mlp.down_proj")


def test_fold_is_an_equivalence_of_the_block():
    """Wrong pairing or direction of a fold changes the block's function (one group folded the
    wrong way: relative error 1.97); the right folds leave only the fp32 roundings of the folded
    vectors (simulated worst case over 200 draws of lognormal scales: 6.0e-8, so 1e-6 leaves 16x)."""
    _dev()
    p = f"{L}.0"
    T = block_tensors(p, 64, 128, 64, torch.float32, seed=11, bias=True)
    S = block_stats(p, 64, 128, seed=12)
    (block,) = plan_of(T, "qwen2")
    assert all(g.foldable for g in block.groups.values())
    out = quantizer().quantize_block(T, S, block)
    assert all(g["folded"] for g in out["groups"].values())
    assert set(out["folded"]) == {f"{p}.input_layernorm.weight", f"{p}.post_attention_layernorm.weight",
                                  f"{p}.self_attn.v_proj.bias"}
    src = {k: v.double() for k, v in T.items()}
    new = dict(src)
    sc = {k: v.cpu().double() for k, v in out["scales"].items()}
    for name in block.members():
        w = src[name] * sc[name + ".input_scale"][None, :]
        if name + ".row_scale" in sc:
            w = w / sc[name + ".row_scale"][:, None]
        new[name] = w
    for name, t in out["folded"].items():
        new[name] = t.cpu().double()
    assert any(not torch.equal(sc[m + ".input_scale"], torch.ones_like(sc[m + ".input_scale"]))
               for m in block.members())
    x = torch.randn(16, 64, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    y0, y1 = forward64(x, src, p, heads=4), forward64(x, new, p, heads=4)
    err = float((y1 - y0).norm() / y0.norm())
    print(f"fold equivalence: relative Frobenius error {err:.3e}")
    assert err <= 1e-6


@pytest.fixture(scope="module")
def tiny_llama(tmp_path_factory):
    """A 2-layer Llama directory (layer 0 MHA, layer 1 GQA) with statistics for every linear."""
    d = tmp_path_factory.mktemp("tiny_llama")
    g = torch.Generator().manual_seed(21)
    tensors = {"model.embed_tokens.weight": torch.randn(256, 128, generator=g).bfloat16(),
               "model.norm.weight": torch.ones(128).bfloat16(),
               "lm_head.weight": torch.randn(256, 128, generator=g).bfloat16()}
    stats = {}
    for i, kv in enumerate((128, 64)):
        tensors.update(block_tensors(f"{L}.{i}", 128, 256, kv, torch.bfloat16, seed=30 + i))
        stats.update(block_stats(f"{L}.{i}", 128, 256, seed=40 + i))
    # a linear inside a block that belongs to no layer group: RTN, its statistics unused
    tensors[EXTRA] = (torch.randn(128, 128, generator=g) * 0.05).bfloat16()
    stats[EXTRA] = stats[f"{L}.1.self_attn.o_proj.weight"]
    save_file(tensors, str(d / "model.safetensors"))
    with open(d / "config.json", "w") as f:
        json.dump({"model_type": "llama", "hidden_size": 128}, f)
    flat = {}
    for name, (xm, xs) in stats.items():
        flat[name + ".x_mean"], flat[name + ".x_sq"] = xm.clone(), xs.clone()
    stats_path = str(tmp_path_factory.mktemp("tiny_llama_stats") / "stats.safetensors")   # not a model file
    save_file(flat, stats_path)
    return str(d), stats_path, tensors


@pytest.mark.parametrize("clip", [False, True], ids=["rtn", "act_clip"])
def test_cli_fold_scales_end_to_end(tiny_llama, tmp_path, clip):
    from awq_quantizer.main import load_act_stats, main
    _dev()
    d, p, tensors = tiny_llama
    base = ["--model_id", d, "--log_level", "ERROR", "--group_size", "32", "--device", "cuda:0"]
    awq = ["--scale_method", "awq", "--act_stats", p, "--output_format", "autoawq"]
    out = tmp_path / "out"
    assert main(base + ["--output_dir", str(out)] + awq + ["--fold_scales"] + (["--act_clip"] if clip else [])) == 0
    st = load_file(str(out / "model.safetensors"))
    side = load_file(str(out / "awq_scales.safetensors"))
    q = quantizer()
    S = load_act_stats(p)
    ckw = {"clip": True, "clip_grid": 20, "clip_max_shrink": 0.5} if clip else {}
    keys, linears = set(), set()
    for block in plan_of(tensors):
        want = q.quantize_block({n: tensors[n] for n in block.tensor_names()}, S, block, **ckw)
        for name, r in want["results"].items():
            e = q.export_autoawq(r)
            for f in ("qweight", "qzeros", "scales"):
                assert torch.equal(st[name[:-len("weight")] + f], e[f].cpu()), (name, f)
            assert name not in st
            linears.add(name)
        for name, t in want["folded"].items():
            assert same_bits(st[name], t) and not torch.equal(st[name], tensors[name]), name
        for k, v in want["scales"].items():
            assert torch.equal(side[k], v.cpu()), k
        keys |= set(want["scales"])
    plan = plan_of(tensors)
    assert plan.ungrouped == [EXTRA]
    e = q.export_autoawq(q.quantize_packed(tensors[EXTRA].to(torch.device("cuda", 0))))
    for f in ("qweight", "qzeros", "scales"):
        assert torch.equal(st[EXTRA[:-len("weight")] + f], e[f].cpu()), (EXTRA, f)
    linears.add(EXTRA)
    assert set(side) == keys and len(linears) == 15
    assert f"{L}.0.self_attn.v_proj.weight.row_scale" in keys and f"{L}.1.self_attn.v_proj.weight.row_scale" not in keys
    for name in ("model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"):
        assert torch.equal(st[name].view(torch.int16), tensors[name].view(torch.int16)), name
    assert set(st) == {n for n in tensors if n not in linears} | {
        n[:-len("weight")] + f for n in linears for f in ("qweight", "qzeros", "scales")}
    # the configs are those of the plain AutoAWQ export
    plain = tmp_path / "plain"
    assert main(base + ["--output_dir", str(plain), "--output_format", "autoawq"]) == 0
    for f in ("quant_config.json", "config.json"):
        assert json.load(open(out / f)) == json.load(open(plain / f)), f
    assert not os.path.exists(plain / "awq_scales.safetensors")
    # without the flag the refusal stands
    assert main(base + ["--output_dir", str(tmp_path / "refused")] + awq) == 1
