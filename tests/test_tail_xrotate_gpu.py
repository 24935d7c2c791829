"""Hadamard rotation on the GPU: awq_hadamard_rows / awq_hadamard_cols against a dense
float64 kron(M, Sylvester) built here (scipy's Sylvester matrix and a literal Paley construction — never
hadamard_factor), the rotate CLI's output read by the independent float64 forward, and the existing
activation-aware flow on a rotated directory.

Model bounds.  e of the rotated fp32 directory <= 1e-5: the geometric mean of the host float64 rotation
rounded to fp32 (3.7e-8) and the smallest mutation (a norm weight kept where ones belong, 3.8e-3); the
test recomputes both ends and fails if they move past 1e-6 / 1e-4.  bf16: e <= 2 x the e of the host
float64 rotation rounded to bf16 (W diag(g) is rounded once where the source rounds it never).

16-bit clause (every element within one ulp of the rounded reference, at most 1 % differing): an output
that cancels to nearly zero has a 16-bit ulp below the fp32 error of its sum, which is why the kernels
add 16-bit matrices in fp64.  Measured on the MI355X: worst 1 ulp, differing share 0 .. 2.4e-4."""
import functools
import json
import math

import pytest
import torch
from safetensors.torch import load_file, save_file
from scipy.linalg import hadamard as sylvester

import model_cases as mc
from checkpoint_reader import read_checkpoint
from test_gpu_calibrate import calib_ids

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
RESIDUES = {11: (1, 3, 4, 5, 9), 19: (1, 4, 5, 6, 7, 9, 11, 16, 17), 13: (1, 3, 4, 9, 10, 12)}

ROWS = [(3, 32, 32, 1), (67, 128, 128, 1), (2, 512, 512, 1), (2, 1024, 1024, 1), (1, 8192, 8192, 1), (3, 256, 64, 1),
        (2, 192, 192, 12), (2, 320, 320, 20), (2, 896, 896, 28)]
COLS = [(128, 72, 128, 1), (1024, 8, 1024, 1), (4096, 264, 4096, 1), (256, 40, 64, 1), (896, 40, 896, 28)]


def paley(m: int) -> torch.Tensor:
    """Paley I of order q + 1 (q = 11, 19) and Paley II of order 2 (q + 1) (q = 13), entry by entry."""
    q = {12: 11, 20: 19, 28: 13}[m]
    s = [[0] * (q + 1) for _ in range(q + 1)]
    for i in range(q + 1):
        for j in range(q + 1):
            if i == 0 and j > 0:
                s[i][j] = 1
            elif j == 0 and i > 0:
                s[i][j] = -1 if m != 28 else 1
            elif i != j and i and j:
                s[i][j] = 1 if (i - j) % q in RESIDUES[q] else -1
    if m != 28:
        return torch.tensor([[s[i][j] + (i == j) for j in range(m)] for i in range(m)], dtype=torch.float64)
    block = {0: ((1, -1), (-1, -1)), 1: ((1, 1), (1, -1)), -1: ((-1, -1), (-1, 1))}
    return torch.tensor([[block[s[i // 2][j // 2]][i % 2][j % 2] for j in range(m)] for i in range(m)],
                        dtype=torch.float64)


def dense_reference(x: torch.Tensor, L: int, m: int, pre) -> torch.Tensor:
    """x float64 [R, K]: every L-segment of (x * pre) times kron(M, H_P) / sqrt(L), P = a b split as
    kron(H_a, H_b) past 1024 so that no 8192 x 8192 matrix is formed."""
    R, K = x.shape
    P = L // m
    b = min(P, 1024)
    M = paley(m) if m > 1 else torch.ones(1, 1, dtype=torch.float64)
    Ha, Hb = (torch.tensor(sylvester(n), dtype=torch.float64) for n in (P // b, b))
    y = (x * pre if pre is not None else x).reshape(R, K // L, m, P // b, b)
    return (torch.einsum("rsjap,jJ,aA,pB->rsJAB", y, M, Ha, Hb) / math.sqrt(L)).reshape(R, K)


def ordered(t: torch.Tensor) -> torch.Tensor:
    """16-bit floats as integers in value order (one step = one ulp)."""
    v = t.view(torch.int16).to(torch.int32)
    return torch.where(v < 0, -(v & 0x7FFF), v)


def check(out: torch.Tensor, ref: torch.Tensor, L: int, m: int, dtype) -> None:
    """out, ref [R, K] with the segments along the last axis."""
    if dtype == torch.float32:
        err = (out.double() - ref).reshape(-1, L).norm(dim=1)
        bound = (math.log2(L) + m + 4) * 2.0 ** -24 * ref.reshape(-1, L).norm(dim=1)
        print(f"worst segment error / bound: {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
    else:
        steps = (ordered(out) - ordered(ref.to(dtype))).abs()
        print(f"differing share: {float((steps > 0).double().mean()):.2e}, worst {int(steps.max())} ulp")
        assert int(steps.max()) <= 1 and float((steps > 0).double().mean()) <= 0.01


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("with_pre", [False, True], ids=["plain", "pre"])
@pytest.mark.parametrize("axis,shape", [("rows", c) for c in ROWS] + [("cols", c) for c in COLS],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_transform_against_dense_float64(axis, shape, with_pre, dt):
    from awq_quantizer.rotation import hadamard_transform
    dtype, dev = DTYPES[dt], torch.device("cuda", 0)
    L, m = shape[2], shape[3]
    g = torch.Generator().manual_seed(3 + sum(shape) + with_pre)
    R, K = (shape[0], shape[1]) if axis == "rows" else (shape[1], shape[0])     # segments along the last axis of x
    x = torch.randn(R, K, generator=g).to(dtype)
    pre = (torch.rand(K, generator=g) + 0.5) * (torch.randint(0, 2, (K,), generator=g) * 2 - 1) if with_pre else None
    ref = dense_reference(x.double(), L, m, None if pre is None else pre.double())
    if axis == "rows":
        out = hadamard_transform(x.to(dev), -1, length=L, pre=pre).cpu()
    else:
        out = hadamard_transform(x.t().contiguous().to(dev), 0, length=L, pre=pre).cpu().t()
    assert out.dtype == dtype
    check(out.contiguous(), ref, L, m, dtype)


# ------------------------------------------------------------------ the model
def host_rotation(fx, heads: bool, seed: int = 0):
    """The rotation of the module docstring in float64 with dense matrices."""
    h, hd = fx.config["hidden_size"], fx.config["head_dim"] if fx.config.get("head_dim") else 32
    d = (torch.randint(0, 2, (h,), generator=torch.Generator().manual_seed(seed)) * 2 - 1).double()
    Q = d[:, None] * torch.tensor(sylvester(h), dtype=torch.float64) / math.sqrt(h)
    Hd = torch.tensor(sylvester(hd), dtype=torch.float64) / math.sqrt(hd)
    s, out = fx.source, {}
    for n, w in s.items():
        p = n.rsplit(".", 3)[0]
        if n.endswith("norm.weight"):
            out[n] = torch.ones_like(w)
        elif n == "model.embed_tokens.weight":
            out[n] = w @ Q
        elif n == "lm_head.weight":
            out[n] = w * s["model.norm.weight"] @ Q
        elif n.endswith(("q_proj.weight", "k_proj.weight", "v_proj.weight")):
            out[n] = w * s[p + ".input_layernorm.weight"] @ Q
        elif n.endswith(("gate_proj.weight", "up_proj.weight")):
            out[n] = w * s[p + ".post_attention_layernorm.weight"] @ Q
        elif n.endswith(("o_proj.weight", "down_proj.weight")):
            out[n] = Q.T @ w
        else:
            out[n] = w
        if heads and n.endswith("v_proj.weight"):
            out[n] = torch.block_diag(*[Hd.T] * (w.shape[0] // hd)) @ out[n]
        if heads and n.endswith("v_proj.bias"):
            out[n] = w @ torch.block_diag(*[Hd] * (w.shape[0] // hd))
        if heads and n.endswith("o_proj.weight"):
            out[n] = out[n] @ torch.block_diag(*[Hd] * (w.shape[1] // hd))
    return out


@functools.lru_cache(maxsize=None)
def host_ends(arch: str, heads: bool):
    """(e of the host rotation rounded to fp32, to bf16, e with one source norm weight kept)."""
    fx = mc.fixture(arch)
    rot = host_rotation(fx, heads)
    norm = "model.layers.0.input_layernorm.weight"
    return (fx.e({k: v.float() for k, v in rot.items()}), fx.e({k: v.bfloat16() for k, v in rot.items()}),
            fx.e({**rot, norm: fx.source[norm]}))


@pytest.fixture(scope="module")
def model_dirs(tmp_path_factory):
    dirs = {}
    for arch in mc.ARCHS:
        fx, d = mc.fixture(arch), tmp_path_factory.mktemp(f"src_{arch}")
        save_file(dict(fx.state), str(d / "model.safetensors"), metadata={"format": "pt"})
        (d / "config.json").write_text(json.dumps(fx.config))
        dirs[arch] = str(d)
    return dirs


@pytest.mark.parametrize("dt,heads", [("float32", False), ("float32", True), ("bfloat16", True)])
@pytest.mark.parametrize("arch", mc.ARCHS)
def test_rotated_directory_computes_the_same_function(model_dirs, tmp_path, arch, dt, heads):
    from awq_quantizer import rotate
    fx, out = mc.fixture(arch), str(tmp_path / "rot")
    assert rotate.main(["--model_id", model_dirs[arch], "--output_dir", out, "--dtype", dt, "--device", "cuda:0",
                        "--log_level", "ERROR"] + (["--rotate_heads"] if heads else [])) == 0
    state = load_file(out + "/model.safetensors")
    e = fx.e(state)
    e32, e16, e_mut = host_ends(arch, heads)
    print(f"{arch} {dt} heads={heads}: e {e:.3g}; host fp32 {e32:.3g}, bf16 {e16:.3g}, mutation {e_mut:.3g}; "
          f"ratio to the host end {e / (e32 if dt == 'float32' else e16):.3f}")
    assert e32 <= 1e-6 and e_mut >= 1e-4
    assert e <= (1e-5 if dt == "float32" else 2 * e16)
    assert all(v.dtype == getattr(torch, dt) for v in state.values()) and set(state) == set(fx.names)
    for n in fx.names:
        if n.endswith("norm.weight"):
            assert torch.equal(state[n], torch.ones_like(state[n])), n
    info = json.load(open(out + "/rotation.json"))
    listed = [n for names in info["tensors"].values() for n in names]
    assert sorted(listed) == sorted(fx.names) and (info["h"], info["m"], info["k"], info["heads"]) == (128, 1, 7, heads)
    assert json.load(open(out + "/config.json"))["tie_word_embeddings"] is False


def test_activation_aware_flow_runs_on_a_rotated_directory(model_dirs, tmp_path):
    from awq_quantizer import calibrate, rotate
    from awq_quantizer.main import main
    fx, ids, es = mc.fixture("llama"), str(tmp_path / "ids.safetensors"), {}
    save_file({"input_ids": calib_ids("llama")}, ids)
    rot = str(tmp_path / "rot")
    assert rotate.main(["--model_id", model_dirs["llama"], "--output_dir", rot, "--rotate_heads", "--device", "cuda:0",
                        "--log_level", "ERROR"]) == 0
    for name, src in (("rotated", rot), ("source", model_dirs["llama"])):
        stats, out = str(tmp_path / f"{name}_stats.safetensors"), str(tmp_path / f"{name}_out")
        assert calibrate.main(["--model_id", src, "--output", stats, "--input_ids", ids, "--device", "cuda:0",
                               "--log_level", "ERROR"]) == 0
        assert main(["--model_id", src, "--output_dir", out, "--log_level", "ERROR", "--group_size", "32", "--device",
                     "cuda:0", "--output_format", "autoawq", "--scale_method", "awq", "--fold_scales", "--act_stats",
                     stats]) == 0
        state, info = read_checkpoint(out)
        assert set(info["quantized"]) == set(fx.quantized_names("autoawq"))
        es[name] = fx.e(state)
    print(f"llama gs32 W4 e: rotated {es['rotated']:.4g}, source {es['source']:.4g}, ratio {es['rotated'] / es['source']:.3f}")
    assert math.isfinite(es["rotated"]) and math.isfinite(es["source"])
