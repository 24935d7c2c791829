"""Records tests/golden/calib/rope_llama3.json: the llama3-scaled RoPE inverse frequencies of two
configs (head_dim 64 and 128) from transformers' own ROPE_INIT_FUNCTIONS["llama3"].  Run by hand
on a CPU with transformers installed (`python tests/golden/make_golden_rope.py`); no test runs it.
tests/test_calibrate_host.py compares awq_quantizer.calibration.rope_inv_freq with the recorded
values always, and with transformers itself when it is importable.

Per case: the config.json keys the calibration forward reads, and inv_freq as the exact fp32
values (hex of the bits, and the decimal for a reader)."""
import json
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [
    # Llama-3.2-1B's geometry: head_dim 64
    dict(hidden_size=2048, num_attention_heads=32, num_key_value_heads=8, head_dim=64,
         max_position_embeddings=131072,
         rope_parameters=dict(rope_type="llama3", rope_theta=500000.0, factor=32.0, low_freq_factor=1.0,
                              high_freq_factor=4.0, original_max_position_embeddings=8192)),
    # Llama-3.1-8B's geometry: head_dim 128
    dict(hidden_size=4096, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
         max_position_embeddings=131072,
         rope_parameters=dict(rope_type="llama3", rope_theta=500000.0, factor=8.0, low_freq_factor=1.0,
                              high_freq_factor=4.0, original_max_position_embeddings=8192)),
]


def main():
    import transformers
    from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
    out = {"transformers_version": transformers.__version__, "cases": []}
    for kw in CASES:
        config = transformers.LlamaConfig(vocab_size=256, intermediate_size=256, num_hidden_layers=1, **kw)
        inv, factor = ROPE_INIT_FUNCTIONS["llama3"](config, "cpu")
        assert factor == 1.0 and inv.dtype.is_floating_point and inv.numel() == kw["head_dim"] // 2
        vals = [float(v) for v in inv.float()]
        out["cases"].append({"config": {"model_type": "llama", "vocab_size": 256, "num_hidden_layers": 1, **kw},
                             "inv_freq_bits": [struct.pack(">f", v).hex() for v in vals],
                             "inv_freq": vals})
    os.makedirs(os.path.join(HERE, "calib"), exist_ok=True)
    with open(os.path.join(HERE, "calib", "rope_llama3.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(f"recorded {len(out['cases'])} cases from transformers {transformers.__version__}")


if __name__ == "__main__":
    main()
