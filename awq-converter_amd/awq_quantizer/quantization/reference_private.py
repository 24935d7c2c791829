"""The reference's private methods (awq.py:130-374) behind AWQQuantizer's methods of the same names.

Subclasses and callers of the reference reach into these; they keep the
reference's signatures, result dtypes and shapes (pinned bit for bit by
tests/test_private_methods.py against 1 024 + 2 668 + 4 484 calls of the reference) and
run on the HIP kernels: awq_group_params_ex (scale / zero point of every group in the
input dtype's own arithmetic), awq_apply_params_ex (element-wise quantize / dequantize with
given parameters) and awq_quantize_groups.  They are the reference's round-to-nearest
whatever scale_method says (the clip search is reached through quantize / quantize_packed).
Results are placed where the reference places them (q.device; _compute_scale_zp_for_group:
the input's device), and computed the way torch computes them THERE: the reference moves its
tensors to self.device, whose torch kernels differ from the CPU's in four places — a GPU
divides by a Python int as a product with its reciprocal (the scale, awq.py:202), clamps -0
to +0 (awq.py:211, 248), converts a one-element device parameter to the op dtype first
(awq.py:245, 282) and converts a NaN to int32 as 0 (awq.py:367).  The public API (quantize,
quantize_packed, dequantize, ...) always gives the reference CPU awq.py's bits (north_star).

Every function takes the quantizer as `q`.
"""
import math
from typing import Tuple

import torch

from .. import _hip
from ..layout import rows_k

_EMPTY_MIN = ("min(): Expected reduction dim to be specified for input.numel() == 0. "
              "Specify the reduction dim with the 'dim' argument.")


def home(q, t: torch.Tensor) -> torch.Tensor:
    """`t` where the reference leaves a result: q.device."""
    return t.to(q.device) if q.device.startswith("cuda") else t.cpu()


def torch_gpu(q) -> bool:
    """The reference would evaluate on a GPU (q.device is a CUDA device)."""
    return q.device.startswith("cuda")


def home_device(q) -> torch.device:
    """Where the reference's tensor.to(self.device) puts a tensor (awq.py:141, 233, 303)."""
    return q.compute_device() if torch_gpu(q) else torch.device("cpu")


def on_gpu(q, tensor: torch.Tensor) -> torch.Tensor:
    """The checked input, contiguous on the compute device."""
    q._check_input(tensor)
    return tensor.detach().to(q.compute_device()).contiguous()


def compute_scale_zp_for_group(q, tensor: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """awq.py:173-213: (scale, zero_point) of the whole tensor as one group, 0-d tensors
    of its dtype (zero_point = 0 when symmetric), on the input's device and computed the way
    torch computes there (the reference does not move this method's input)."""
    q._check_mode()
    x = on_gpu(q, tensor)
    n = x.numel()
    if n == 0:
        raise RuntimeError(_EMPTY_MIN)
    s, z = _hip.group_params(x, 1, n, n, q.bits, q.symmetric, torch_gpu=tensor.is_cuda)
    return s.reshape(()).to(tensor.device, tensor.dtype), z.reshape(()).to(tensor.device, tensor.dtype)


def calculate_scale_zp(q, tensor: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """awq.py:130-171: one group for the whole tensor (dim <= 1 or per_channel=False),
    else one per dim-0 channel ([C] tensors of the input dtype)."""
    if tensor.dim() <= 1 or not q.per_channel:
        s, z = q._compute_scale_zp_for_group(tensor.to(home_device(q)))   # awq.py:141
        return s, z
    q._check_mode()
    C = tensor.size(0)
    if C == 0:
        raise RuntimeError("stack expects a non-empty TensorList")
    x = on_gpu(q, tensor)
    K = x.numel() // C
    if K == 0:
        raise RuntimeError(_EMPTY_MIN)
    s, z = _hip.group_params(x, C, K, K, q.bits, q.symmetric, torch_gpu=torch_gpu(q))
    return home(q, s.reshape(C).to(tensor.dtype)), home(q, z.reshape(C).to(tensor.dtype))


def sub_check(a: torch.dtype, b: torch.dtype) -> None:
    """ATen's sub_check: `-` with a bool operand raises (the meta ops of apply skip it)."""
    if a == torch.bool and b == torch.bool:
        raise RuntimeError("Subtraction, the `-` operator, with two bool tensors is not supported. "
                           "Use the `^` or `logical_xor()` operator instead.")
    if a == torch.bool or b == torch.bool:
        raise RuntimeError("Subtraction, the `-` operator, with a bool tensor is not supported. "
                           "If you are trying to invert a mask, use the `~` or `logical_not()` operator "
                           "instead.")


def param_words(p: torch.Tensor, dev: torch.device) -> Tuple[torch.Tensor, int]:
    """A parameter on the device as 8-byte words and its kind: 0 = float64 values (exact for
    every float dtype), 1 = int64 values for integer / bool parameters, 2 = uint64 (their
    bits) — exact whatever their magnitude."""
    if p.is_floating_point():
        return p.detach().to(dev, torch.float64), 0
    if p.dtype == torch.uint64:
        return p.detach().to(dev).view(torch.int64).view(torch.float64), 2
    return p.detach().to(dev, torch.int64).view(torch.float64), 1


def apply(q, tensor: torch.Tensor, scale, zero_point, mode: int) -> torch.Tensor:
    """_quantize_tensor (mode 0) / _dequantize_tensor (mode 1) as the reference evaluates
    awq.py:245 / awq.py:282: the per-channel reshape of awq.py:237-242 / 274-279, then
    torch's broadcasting and type promotion, for tensors and parameters of any float,
    integer or bool dtype.  The two ops' result dtypes come from torch's own promotion
    (meta tensors: no data, no compute; torch.result_type for the promotion errors the meta
    ops skip); the arithmetic runs in awq_apply_params_ex in those dtypes.  A one-element
    parameter of a bf16 / fp16 op enters at its own value when the reference would evaluate
    on the CPU (device="cpu": ATen's CPU kernels read its original value) and converted to
    the op dtype first when it would evaluate on the GPU (device="cuda": a device tensor,
    cast like any operand; and there clamp(-0, 0, qmax) is +0, the GPU clamp's IEEE maximum).  Pinned by tests/golden/golden_promote.* and
    golden_promote_int.* (reference calls on the CPU: float / int32 tensors with promoting
    parameters; int64 / int16 / int8 / uint8 / bool / uint16 / uint32 / uint64 tensors with
    float, integer and bool parameters) and, for device="cuda", by torch's own CUDA
    evaluation of the same expressions (tests/test_private_methods.py)."""
    scale, zero_point = torch.as_tensor(scale), torch.as_tensor(zero_point)
    if scale.is_complex() or zero_point.is_complex() or tensor.is_complex():
        raise NotImplementedError("complex tensors or parameters")
    per_ch = q.per_channel and tensor.dim() > 1 and scale.dim() == 1
    if per_ch:                                   # awq.py:238-242 (same errors as the reference)
        shp = [scale.size(0)] + [1] * (tensor.dim() - 1)
        scale, zero_point = scale.reshape(shp), zero_point.reshape(shp)
    meta = lambda t: torch.empty(t.shape, dtype=t.dtype, device="meta")
    x_m, s_m, z_m = meta(tensor), meta(scale), meta(zero_point)
    if mode == 1:
        sub_check(tensor.dtype, zero_point.dtype)
    torch.result_type(x_m, s_m if mode == 0 else z_m)       # torch's promotion errors
    first = (x_m / s_m) if mode == 0 else (x_m - z_m)       # torch's broadcasting / promotion
    torch.result_type(first, z_m if mode == 0 else s_m)
    res = (first + z_m) if mode == 0 else (first * s_m)
    d1, d2, shape = first.dtype, res.dtype, tuple(res.shape)
    for dt in (d1, d2):
        if dt not in _hip.APPLY_OP_DTYPE:                    # torch has no such kernel either
            raise NotImplementedError(f"\"add_stub\" not implemented for '{q._UNSIGNED_NAMES.get(dt, dt)}'")
    if tensor.dtype not in _hip.APPLY_DTYPE:
        raise NotImplementedError(f"tensor dtype {tensor.dtype}")
    dev = q.compute_device()
    if math.prod(shape) == 0:
        return home(q, torch.empty(shape, dtype=d2, device=dev))
    x = tensor.detach().to(dev).contiguous()
    s64, s_kind = param_words(scale, dev)
    z64, z_kind = param_words(zero_point, dev)
    n = x.numel()
    if shape == tuple(tensor.shape) and scale.numel() == 1 and zero_point.numel() == 1:
        rows, K, L = 1, n, n                     # one parameter pair for the whole tensor
        s64, z64 = s64.reshape(1), z64.reshape(1)
    elif shape == tuple(tensor.shape) and per_ch:
        rows = tensor.size(0)                    # one pair per dim-0 channel
        K = n // rows
        L = max(K, 1)
        s64, z64 = s64.reshape(rows), z64.reshape(rows)
    else:                                        # any other broadcast: one pair per element
        x = x.expand(shape).contiguous()
        s64, z64 = s64.expand(shape).reshape(-1), z64.expand(shape).reshape(-1)
        rows, K, L = 1, x.numel(), 1
    cpu_scalars = not torch_gpu(q)
    flags = ((_hip.APPLY_SCALE_ONE_ELEMENT if cpu_scalars and scale.numel() == 1 else 0) |
             (0 if cpu_scalars else _hip.APPLY_IEEE_CLAMP) |
             (_hip.APPLY_ZERO_ONE_ELEMENT if cpu_scalars and zero_point.numel() == 1 else 0) |
             (_hip.APPLY_SCALE_INT if s_kind else 0) | (_hip.APPLY_ZERO_INT if z_kind else 0) |
             (_hip.APPLY_SCALE_UNSIGNED if s_kind == 2 else 0) | (_hip.APPLY_ZERO_UNSIGNED if z_kind == 2 else 0))
    out = _hip.apply_params(x, rows, K, L, s64.contiguous(), z64.contiguous(), q.qmin, q.qmax, mode, d1, d2,
                            flags)
    return home(q, out.reshape(shape))


def quantize_per_group(q, tensor: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """awq.py:286-374: (tensor_q int32 of the input shape, scales fp32 [rows, G],
    zero_points fp32 [rows, G]); tensors smaller than one group take
    _calculate_scale_zp + _quantize_tensor (awq.py:297-300)."""
    if tensor.numel() < q.group_size:
        scale, zero_point = q._calculate_scale_zp(tensor)
        return q._quantize_tensor(tensor, scale, zero_point), scale, zero_point
    q._check_mode()
    x = on_gpu(q, tensor)
    rows, K = rows_k(x.shape)
    L = q.group_size
    gpu = torch_gpu(q)
    s, z = _hip.group_params(x, rows, K, L, q.bits, q.symmetric, torch_gpu=gpu)
    if not gpu:
        tq = torch.empty(rows * K, dtype=torch.int32, device=x.device)
        _hip.quantize_groups(x, rows, K, L, q.bits, q.symmetric, tensor_q=tq)
    else:
        # awq.py:356-367 as the GPU evaluates it: each group quantized with its own 0-d
        # parameters (awq_apply_params_ex, GPU clamp), the float result stored into the
        # int32 tensor_q by torch's own GPU conversion (NaN -> 0; the reference's setitem)
        tqf = _hip.apply_params(x.reshape(-1), rows, K, L, s.reshape(-1).contiguous(), z.reshape(-1).contiguous(),
                                q.qmin, q.qmax, 0, x.dtype, x.dtype, _hip.APPLY_IEEE_CLAMP)
        tq = tqf.to(torch.int32)
    return home(q, tq.reshape(tensor.shape)), home(q, s.float()), home(q, z.float())
