"""Ragged multi-tensor launch: many tensors, one kernel (include/awq_hip.h
awq_plan_ragged / awq_quantize_ragged).

A model's tensor set (e.g. opt-125m: 196 tensors, 110 of them 768-element biases) is
quantized by ONE launch of the streaming kernel over all tensors' tiles instead of one
launch (or, in the reference, ~20 ATen dispatches per 128-element group,
awq.py:345-368) per tensor.  The descriptor table is planned once on the host,
uploaded once, and can be re-launched any number of times (bench.py does).
"""
from typing import Dict, Optional

import torch

from .. import _hip
from ..layout import device_input, packed_shapes, result_meta, rows_k

REFERENCE_KEYS = ("tensor_q", "scales", "zero_points", "bits", "group_size", "symmetric")   # awq.py:409-416


class PackedBatch:
    """Device-resident inputs + packed outputs of one ragged launch.

    inputs: name -> contiguous device tensor ([rows, ...] or 1-D), K % group_size == 0, all
    bf16, all fp16 or all fp32; group_size 32, 64, 128 or 256 (one per batch).
    parity=True additionally produces the reference's unpacked int32 tensor_q and
    zero_points (6.05 B/element of output traffic instead of 0.52).
    use_block_table: upload the per-workgroup tensor table (awq_plan_block_tensor; 4 B per
    4 tiles) so no wave has to search the descriptors.
    search: (n_grid, n_candidates) runs the clip search of scale_method="search" in the same
    one launch (awq_quantize_ragged_search; the bits of awq_quantize_search per tensor).
    """

    def __init__(self, inputs: Dict[str, torch.Tensor], bits: int = 4, symmetric: bool = False,
                 parity: bool = False, packed: bool = True, use_block_table: bool = True, group_size: int = 128,
                 search: Optional[tuple] = None):
        if not inputs:
            raise ValueError("PackedBatch needs at least one tensor")
        self.bits, self.symmetric, self.parity = bits, bool(symmetric), parity
        self.group_size = gs = int(group_size)
        self.search = tuple(search) if search is not None and search[1] > 1 else None
        self.names = list(inputs)
        first = next(iter(inputs.values()))
        dev, self.dtype = first.device, first.dtype
        if self.dtype not in (torch.bfloat16, torch.float16, torch.float32):
            raise ValueError(f"PackedBatch takes bf16, fp16 or fp32 tensors, got {self.dtype}")
        _hip.require_device(dev)
        self.device = dev
        self.inputs = inputs
        self.out = {}
        descs = []
        for name in self.names:
            x = inputs[name]
            if x.device != dev or x.dtype != self.dtype or not x.is_contiguous():
                raise ValueError(f"{name}: inputs must be contiguous {self.dtype} tensors on {dev} (one dtype "
                                 f"per batch)")
            sh = packed_shapes(x.shape, gs, bits)     # padded rows: the tail group counts (awq.py:337-339)
            rows, K = sh["rows"], sh["K"]
            if not _hip.ragged_eligible(x.dtype, rows, K, gs):
                raise ValueError(f"{name}: shape {tuple(x.shape)} is not eligible for a ragged launch "
                                 f"(group_size {gs})")
            o = {"scales": torch.empty(sh["scales"], dtype=torch.float16, device=dev)}
            if packed:
                o["qweight"] = torch.empty(sh["qweight"], dtype=torch.int32, device=dev)
                o["qzeros"] = torch.empty(sh["qzeros"], dtype=torch.int32, device=dev)
            if parity:
                o["tensor_q"] = torch.empty(x.shape, dtype=torch.int32, device=dev)
                o["zero_points"] = torch.empty(sh["scales"], dtype=torch.int32, device=dev)
            self.out[name] = o
            p = lambda k: o[k].data_ptr() if k in o else None
            descs.append(_hip.TensorDesc(x.data_ptr(), rows, K, p("qweight"), p("qzeros"), p("scales"),
                                         p("tensor_q"), p("zero_points"), 0, 0))
        self.total_tiles = _hip.plan_ragged(descs, bits, gs)
        self.flags = _hip.ragged_flags(descs, gs)       # padded rows -> the row-tile kernel instance
        self.descs = descs
        # the tables go up asynchronously on the construction stream (pinned H2D); `ready`
        # orders any other stream run() is given after them
        self._stream0 = torch.cuda.current_stream(dev)
        self.descs_dev = _hip.descs_to_device(descs, dev)
        self.block_tensor = _hip.plan_block_tensor(descs, self.total_tiles, dev) if use_block_table else None
        self._ready = torch.cuda.Event()
        self._ready.record(self._stream0)
        self.elements = sum(inputs[n].numel() for n in self.names)

    def run(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if s != self._stream0:       # the kernel reads the uploaded tables (raw output pointers)
            s.wait_event(self._ready)
        _hip.quantize_ragged(self.descs_dev, len(self.descs), self.total_tiles, self.bits, self.symmetric,
                             s.cuda_stream, self.block_tensor, self.dtype, self.group_size, self.flags,
                             search=self.search)

    def results(self) -> Dict[str, Dict[str, torch.Tensor]]:
        return {name: dict(self.out[name], **result_meta(self.bits, self.group_size, self.symmetric,
                                                         self.inputs[name].shape))
                for name in self.names}

    def algorithmic_bytes(self) -> int:
        """HBM bytes one launch must move: bf16 in + packed out (+ parity outputs)."""
        b = 0
        for name in self.names:
            b += self.inputs[name].numel() * self.inputs[name].element_size()
            for t in self.out[name].values():
                b += t.numel() * t.element_size()
        return b


def quantize_model_batched(q, tensors: Dict[str, torch.Tensor], packed: bool) -> Dict[str, Dict[str, torch.Tensor]]:
    """AWQQuantizer.quantize_model_packed (packed) / quantize_model_device(packed=False): the
    ragged-eligible tensors in one PackedBatch per dtype, the rest one by one, failures logged
    and skipped, results in input order.  The two differ in when a tensor is refused and when
    the one-by-one tensors run; each branch on `packed` below is one such difference."""
    one = q.quantize_packed if packed else q._quantize_device
    out, eligible, rest = {}, {}, {}

    def single(name, t):
        try:
            out[name] = one(t)
        except Exception as e:
            q.logger.error(f"Error quantizing tensor: {name}, error: {e}")

    if packed:
        q._check_mode()          # raises out of the call; unpacked: per tensor, logged (the reference's skip)
    for name, t in tensors.items():
        try:
            q._check_input(t)
            if not packed:
                q._check_mode()
        except Exception as e:  # reference semantics: skip and continue
            q.logger.error(f"Error quantizing tensor: {name}, error: {e}")
            continue
        if packed and t.numel() < q.group_size:      # (unpacked: quantize()'s small-tensor path)
            q.logger.error(f"Error quantizing tensor: {name}, error: numel < group_size")
            continue
        rows, K = rows_k(t.shape)
        if t.numel() >= q.group_size and _hip.ragged_eligible(t.dtype, rows, K, q.group_size):
            eligible[name] = t
        elif packed:
            rest[name] = t       # after the batches
        else:
            single(name, t)      # before them
    if eligible:
        dev = q.compute_device()
        for dt in (torch.bfloat16, torch.float16, torch.float32):   # one ragged launch per input dtype
            part = {k: device_input(v, dev) for k, v in eligible.items() if v.dtype == dt}
            if not part:
                continue
            try:
                batch = PackedBatch(part, bits=q.bits, symmetric=q.symmetric, parity=not packed, packed=packed,
                                    group_size=q.group_size, search=q._search_args())
                batch.run()
                res = batch.results()
            except Exception as e:   # the batch as a whole failed: every tensor on its own
                q.logger.error(f"ragged launch of {len(part)} tensors failed ({e}); quantizing them one by one")
                if packed:
                    rest.update(part)
                else:
                    for name, t in part.items():
                        single(name, t)
                continue
            for name, r in res.items():
                out[name] = r if packed else {k: r[k] for k in REFERENCE_KEYS}
    for name, t in rest.items():
        single(name, t)
    return {k: out[k] for k in tensors if k in out}
