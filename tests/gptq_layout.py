"""AutoGPTQ's 4-bit layout (desc_act = false) restated with torch on the CPU, from the published
format alone: what tests compare awq_export_gptq / awq_import_gptq against.

Per linear [N = out_features, K = in_features], G = K / group_size:
  qweight int32 [K/8, N]   nibble i of word (r, n) = u[n, 8r + i]
  qzeros  int32 [G, N/8]   nibble i of word (g, c) = zs[g, 8c + i]
  scales  fp16  [G, N]
  g_idx   int32 [K]        k // group_size
u and z' are the project's packed fields (q - qmin: q and z when asymmetric, q + 8 and 8 when
symmetric); zs = (z' - zero_offset) & 15, zero_offset 1 for checkpoint_format "gptq", 0 for
"gptq_v2".  A loader dequantizes w = (u - ((zs + zero_offset) & 15)) * scale[g_idx[k]].
"""
import torch

ZERO_OFFSET = {"gptq": 1, "gptq_v2": 0}


def fields_of(words: torch.Tensor, n: int) -> torch.Tensor:
    """Row-major packed words [R, W] -> the first n 4-bit fields of every row, int64 [R, n]."""
    w = words.to(torch.int64) & 0xFFFFFFFF
    f = torch.stack([(w >> (4 * i)) & 15 for i in range(8)], dim=-1)
    return f.reshape(w.shape[0], -1)[:, :n].contiguous()


def words_of(fields: torch.Tensor) -> torch.Tensor:
    """int fields [R, n] (values 0..15) -> packed int32 words [R, ceil(n/8)], field j of a word at
    bits 4j..4j+3, the unused high fields of the last word 0."""
    R, n = fields.shape
    W = -(-n // 8)
    f = torch.zeros((R, W * 8), dtype=torch.int64)
    f[:, :n] = fields.to(torch.int64) & 15
    f = f.reshape(R, W, 8)
    w = torch.zeros((R, W), dtype=torch.int64)
    for i in range(8):
        w |= f[:, :, i] << (4 * i)
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w)
    return w.to(torch.int32)


def pack(u: torch.Tensor, z: torch.Tensor, scales: torch.Tensor, group_size: int, zero_offset: int) -> dict:
    """Fields u [N, K], zero fields z' [N, G] and fp16 scales [N, G] -> the four GPTQ tensors."""
    N, K = u.shape
    assert N % 8 == 0 and K % 8 == 0 and K % group_size == 0 and z.shape == (N, K // group_size)
    zs = (z.to(torch.int64) - zero_offset) & 15
    return {"qweight": words_of(u.t().contiguous().reshape(K // 8, 8, N).permute(0, 2, 1).reshape(-1, 8))
            .reshape(K // 8, N),
            "qzeros": words_of(zs.t().contiguous()),                  # [G, N] fields -> [G, N/8] words
            "scales": scales.t().contiguous(),
            "g_idx": (torch.arange(K, dtype=torch.int64) // group_size).to(torch.int32)}


def unpack(gptq: dict, zero_offset: int):
    """The four GPTQ tensors -> (u [N, K], z' [N, G], scales [N, G])."""
    K8, N = gptq["qweight"].shape
    u = fields_of(gptq["qweight"].reshape(-1, 1), 8).reshape(K8, N, 8).permute(1, 0, 2).reshape(N, K8 * 8)
    zs = fields_of(gptq["qzeros"], N)                                 # [G, N]
    z = ((zs + zero_offset) & 15).t().contiguous()
    return u.contiguous(), z, gptq["scales"].t().contiguous()


def from_packed(packed: dict, zero_offset: int) -> dict:
    """The helper applied to the project's packed result (row-major qweight / qzeros / scales)."""
    N, K = (int(v) for v in packed["shape"].tolist())
    gs = int(packed["group_size"])
    return pack(fields_of(packed["qweight"].cpu(), K), fields_of(packed["qzeros"].cpu(), K // gs),
                packed["scales"].cpu(), gs, zero_offset)


def to_packed_words(gptq: dict, zero_offset: int) -> dict:
    """The row-major packed words (qweight, qzeros, scales) a GPTQ linear imports to."""
    u, z, sc = unpack(gptq, zero_offset)
    return {"qweight": words_of(u), "qzeros": words_of(z), "scales": sc}


def dequantize(gptq: dict, zero_offset: int) -> torch.Tensor:
    """The published formula, independent of pack / unpack above: per element
    w[n, k] = (u - ((zs + zero_offset) & 15)) * scale[g_idx[k], n] in fp16 arithmetic (an fp16
    difference, exact, times the fp16 scale, rounded to fp16), returned as fp32 [N, K]."""
    qw = gptq["qweight"].to(torch.int64) & 0xFFFFFFFF                 # [K/8, N]
    qz = gptq["qzeros"].to(torch.int64) & 0xFFFFFFFF                  # [G, N/8]
    K8, N = qw.shape
    g_idx = gptq["g_idx"].to(torch.int64)
    k = torch.arange(K8 * 8)
    u = (qw[k // 8, :] >> (4 * (k % 8))[:, None]) & 15                # [K, N]
    n = torch.arange(N)
    zs = (qz[:, n // 8] >> (4 * (n % 8))[None, :]) & 15               # [G, N]
    z = ((zs + zero_offset) & 15)[g_idx, :]                           # [K, N]
    s = gptq["scales"][g_idx, :]                                      # [K, N] fp16
    return ((u - z).to(torch.float16) * s).float().t().contiguous()
