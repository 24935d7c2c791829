"""Records tests/golden/model_<arch>/: three tiny decoder models built from transformers' own
classes, their activation statistics and their float64 logits.  Run by hand on a CPU with
transformers installed (`python tests/golden/make_golden_model.py`); no test runs it — the tests
read the fixtures (tests/test_model_forward_host.py re-derives the logits from the real classes
when transformers is importable, which guards against a stale fixture).

  llama    LlamaForCausalLM    4 heads, 4 kv heads             every layer group foldable
  mistral  MistralForCausalLM  4 heads, 2 kv heads (GQA)       attn_out not foldable
  qwen2    Qwen2ForCausalLM    4 heads, 4 kv heads, qkv bias   attn_out fold reaches v_proj.bias

All: 2 layers, hidden 128, intermediate 256, vocab 256, untied lm_head, 64 positions.  The
architectures differ in eps / theta as well, so a forward that ignores the config fails one.

Weights come from one seeded torch.Generator per architecture: norm weights 1 + 0.2 randn (a
fold into a norm is visible), linears and lm_head 0.05 randn, biases 0.1 randn, embeddings randn
with eight channels scaled by 30 (salient input channels, so the activation-aware search leaves
candidate 0); the same eight channels of v_proj.bias scaled by 30 too (they pass through the
attention unchanged: salient o_proj inputs, so a dropped bias fold is visible).  Every value is
rounded to 8 significant bits (bf16) and anything below 2^-14 in magnitude set to 0: the same
values are then exact in bf16, fp16 and fp32.

Per directory:
  model.safetensors   bf16 state dict
  config.json         config.to_dict()
  stats.safetensors   "<linear weight name>.x_mean" = mean |x|, ".x_sq" = mean x^2 (fp32, summed in
                      fp64) of the input of every nn.Linear, by forward hooks over 4 x 32 tokens
  expect.safetensors  input_ids int64 [2, 24] (drawn apart from the calibration ids) and the float64
                      logits of the float64 model on them
  names.json          state-dict name -> shape

transformers keeps three fp32 islands whatever the model's dtype: RoPE's angles, RMSNorm's variance
and the eager attention's softmax.  float64_model() evaluates the first two by the same formulas
without the casts (theta^(-2i/d) * position -> cos / sin; w * h * rsqrt(mean h^2 + eps)) and takes
torch's scaled_dot_product_attention for the third, so the recorded logits are float64
throughout; everything else is transformers' own code.  float64_model(stock=True) is transformers
untouched: tests/test_model_forward_host.py checks that it agrees with the fixture to what those
fp32 roundings allow, so the replacements changed the precision and nothing else.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ARCHS = ("llama", "mistral", "qwen2")
SALIENT = (3, 17, 31, 45, 64, 78, 101, 120)
COMMON = dict(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
              num_attention_heads=4, max_position_embeddings=64, tie_word_embeddings=False)


def model_class_and_config(arch: str):
    import transformers as T
    if arch == "llama":
        return T.LlamaForCausalLM, T.LlamaConfig(num_key_value_heads=4, rms_norm_eps=1e-5, rope_theta=10000.0,
                                                 **COMMON)
    if arch == "mistral":
        return T.MistralForCausalLM, T.MistralConfig(num_key_value_heads=2, rms_norm_eps=1e-6, rope_theta=10000.0,
                                                     sliding_window=None, **COMMON)
    if arch == "qwen2":
        return T.Qwen2ForCausalLM, T.Qwen2Config(num_key_value_heads=4, rms_norm_eps=1e-6, rope_theta=1000000.0,
                                                 **COMMON)
    raise ValueError(arch)


def exact_in_all_dtypes(t: torch.Tensor) -> torch.Tensor:
    t = t.float().bfloat16().float()                       # 8 significant bits
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def init_state(shapes: dict, seed: int) -> dict:
    g = torch.Generator().manual_seed(seed)
    state = {}
    for name, shape in shapes.items():
        r = torch.randn(shape, generator=g, dtype=torch.float32)
        if "norm" in name:
            t = 1.0 + 0.2 * r
        elif name.endswith(".bias"):
            t = 0.1 * r
            if name.endswith("v_proj.bias"):               # salient o_proj input channels
                t[list(SALIENT)] *= 30.0
        elif "embed_tokens" in name:
            t = r
            t[:, list(SALIENT)] *= 30.0
        else:
            t = 0.05 * r
        state[name] = exact_in_all_dtypes(t)
    return state


def float64_model(cls, config, state: dict, stock: bool = False):
    """The real class in float64 with `state` loaded strictly.  stock=False: the three fp32 islands
    (module docstring) evaluated in float64; stock=True: transformers exactly as it is."""
    config = type(config).from_dict(config.to_dict())
    config._attn_implementation = "eager" if stock else "sdpa"
    model = cls(config).double().eval()
    model.load_state_dict({k: v.double() for k, v in state.items()}, strict=True)
    if stock:
        return model
    theta = float(config.rope_parameters["rope_theta"])
    dim = config.hidden_size // config.num_attention_heads

    def rope64(x, position_ids):
        inv = theta ** (-torch.arange(0, dim, 2, dtype=torch.float64) / dim)
        ang = position_ids[:, :, None].double() * inv[None, None, :]
        emb = torch.cat((ang, ang), dim=-1)
        return emb.cos(), emb.sin()

    def rmsnorm64(mod):
        def fn(h):
            return mod.weight * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + mod.variance_epsilon))
        return fn

    model.model.rotary_emb.forward = rope64
    n = 0
    for mod in model.modules():
        if type(mod).__name__.endswith("RMSNorm"):
            mod.forward = rmsnorm64(mod)
            n += 1
    assert n == 2 * config.num_hidden_layers + 1
    return model


def linear_input_stats(model, ids: torch.Tensor) -> dict:
    sums = {}

    def hook(name):
        def fn(_mod, args):
            x = args[0].detach().double().reshape(-1, args[0].shape[-1])
            a, s, n = sums.get(name, (0.0, 0.0, 0))
            sums[name] = (a + x.abs().sum(0), s + (x * x).sum(0), n + x.shape[0])
        return fn

    handles = [m.register_forward_pre_hook(hook(n + ".weight")) for n, m in model.named_modules()
               if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        model(input_ids=ids)
    for h in handles:
        h.remove()
    out = {}
    for name, (a, s, n) in sums.items():
        out[name + ".x_mean"] = (a / n).float()
        out[name + ".x_sq"] = (s / n).float()
    return out


def make(arch: str, seed: int) -> None:
    from safetensors.torch import save_file
    cls, config = model_class_and_config(arch)
    shapes = {k: tuple(v.shape) for k, v in cls(config).state_dict().items()}
    state = init_state(shapes, seed)
    model = float64_model(cls, config, state)
    g = torch.Generator().manual_seed(seed + 1000)
    calib = torch.randint(0, 256, (4, 32), generator=g)
    ids = torch.randint(0, 256, (2, 24), generator=torch.Generator().manual_seed(seed + 2000))
    stats = linear_input_stats(model, calib)
    with torch.no_grad():
        logits = model(input_ids=ids).logits
    assert logits.dtype == torch.float64
    d = os.path.join(HERE, f"model_{arch}")
    os.makedirs(d, exist_ok=True)
    save_file({k: v.bfloat16() for k, v in state.items()}, os.path.join(d, "model.safetensors"),
              metadata={"format": "pt"})
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(config.to_dict(), f, indent=1, sort_keys=True)
    save_file(stats, os.path.join(d, "stats.safetensors"))
    save_file({"input_ids": ids, "logits": logits.contiguous()}, os.path.join(d, "expect.safetensors"))
    with open(os.path.join(d, "names.json"), "w") as f:
        json.dump({k: list(v) for k, v in shapes.items()}, f, indent=1)
    print(f"{arch}: {len(state)} tensors, max|logits| {float(logits.abs().max()):.4f}")


if __name__ == "__main__":
    for i, arch in enumerate(sys.argv[1:] or ARCHS):
        make(arch, 7000 + 10 * ARCHS.index(arch))
