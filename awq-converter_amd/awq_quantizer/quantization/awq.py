"""
AWQ group quantizer — drop-in for the reference's AWQQuantizer, computed on MI355X.

Reference: shanefitch/AWQ-Converter src/awq_quantizer/quantization/awq.py.
Same constructor signature and defaults (awq.py:29-43), same validation errors
(awq.py:95-112), same result dict (awq.py:409-416, CPU tensors owned by the caller),
same quantize_model skip-and-log behaviour (awq.py:435-457) and dequantize
(awq.py:459-539).  The per-group Python double loop (awq.py:286-374) is replaced by
one launch of the HIP kernels behind include/awq_hip.h; results are bit-identical to
the reference CPU path (tests/test_gpu_parity.py against the oracle and the golden
fixtures).

Extensions (no reference counterpart): quantize_packed / quantize_model_packed keep the
packed int4/int8 words (qweight/qzeros) and fp16 scales on the device for throughput;
scale_method="search" (new value, opt-in) runs the per-group clip search of
include/awq_hip.h awq_quantize_search instead of plain RTN ("mse"/"minmax" stay RTN);
scale_method="awq" (new value, opt-in) adds quantize_layer_group, the activation-aware
per-input-channel scale search of include/awq_hip.h awq_act_* (act_search.py), and
quantize_block, which runs it over the layer groups of a decoder block (block_plan.py) and
folds 1 / s into the ops producing each input (awq_fold_rows); with token samples of a linear's
input, quantization_error(samples=) measures a result at the layer's output and
quantize_layer_group / quantize_block(loss="output") score the search by that error
(include/awq_hip.h awq_output_error).

This module is the class: its state, its checks, the reference API and quantize_packed.  Every
other method is a delegate to a function that takes the quantizer first — reference_private.py
(the reference's private methods), batch.py (whole models), act_search.py (activation-aware),
autoawq.py (AutoAWQ in and out), gptq.py (GPTQ in and out), gptq_round.py (GPTQ's error-compensated
rounding), report.py (the error report) — imported when first called; shapes and result metadata
come from ../layout.py.
"""

from typing import Dict, Optional, Tuple

import torch

from .. import _hip
from ..layout import aligned, groups, packed_shapes, read_meta, result_meta, rows_k
from ..utils.logger import get_logger
from .report import error_report, output_report  # noqa: F401  (imported from here by verify.py and callers)


class AWQQuantizer:
    """
    AWQ Quantizer (group-wise min/max RTN quantization, HIP backend).
    """

    # quantize_layer_group / quantize_block with clip=True: how the clip search scores a shrink.
    # "diag": the x_sq-weighted loss (awq_quantize_clip_scaled); "output": the error at the
    # linear's output on token samples (awq_quantize_clip_output), which needs samples= (or
    # activations=).  A setting of the quantizer, like search_grid: set it on the instance.
    # act_search.quantize_layer_group / quantize_block also take it per call (clip_loss=).
    clip_loss = "diag"

    # quantize_layer_group / quantize_block: how the fields are chosen once the scales are.
    # "nearest": round to nearest; "gptq": every member of a group that has token samples goes
    # through quantize_gptq(w, samples, input_scale=s, damp=gptq_damp) after the scale search (a
    # group without samples rounds to nearest, with a warning; clip=True is refused: the solver
    # moves the ranges the clip chose).  Settings of the quantizer, like clip_loss.
    rounding = "nearest"
    gptq_damp = 0.01

    def __init__(
        self,
        bits: int = 4,
        group_size: int = 128,
        symmetric: bool = True,
        zero_point: str = "minmax",
        percentile: float = 0.99,
        scale_method: str = "mse",
        per_channel: bool = True,
        device: Optional[str] = None,
        logger_name: str = "awq_quantizer",
        logger_level: str = "INFO",
        logger_to_file: bool = False,
        logger_file_path: Optional[str] = None,
        search_grid: int = 20,
        search_max_shrink: float = 0.5,
        duo_scaling: bool = True,
    ):
        self.bits = bits
        self.group_size = group_size
        self.symmetric = symmetric
        self.zero_point = zero_point
        self.percentile = percentile
        # accepted and validated like the reference; "mse" and "minmax" both give the
        # reference's round-to-nearest scales (awq.py:66 stores it, nothing reads it)
        self.scale_method = scale_method
        self.per_channel = per_channel
        # scale_method="search" only: candidates alpha = 1 - i/search_grid,
        # i < int(search_max_shrink * search_grid) (alpha = 1 first: RTN wins ties)
        self.search_grid = search_grid
        self.search_max_shrink = search_max_shrink
        # scale_method="awq" only (quantize_layer_group): search_grid ratios r = i/search_grid,
        # channel scales x_mean^r [/ w_mean^(1-r)] (duo_scaling, AutoAWQ's default)
        self.duo_scaling = duo_scaling

        # device string semantics of awq.py:70-77
        if device is None:
            self.device = "cuda" if torch.cuda.is_available() else "cpu"
        else:
            self.device = device
        if self.device.startswith("cuda") and not torch.cuda.is_available():
            self.device = "cpu"

        self.logger = get_logger(name=logger_name, level=logger_level, to_file=logger_to_file,
                                 file_path=logger_file_path)
        self._validate_parameters()
        self.qmin, self.qmax = self._calculate_qmin_qmax()
        self.logger.info(f"Initialized AWQ Quantizer with bits={bits}, group_size={group_size}, symmetric={symmetric}")
        self.logger.info(f"Quantization range: [{self.qmin}, {self.qmax}]")
        if self.device == "cpu" and torch.cuda.is_available():
            self.logger.info("device='cpu': this build has no CPU path; the HIP kernels run on the current GPU "
                             "and results are returned on the CPU (bit-identical to the reference's CPU results)")
        if self.scale_method == "awq":
            self.logger.info("scale_method='awq': the activation-aware search runs in quantize_layer_group(); "
                             "tensors quantized without activations (quantize, quantize_model) are RTN")

    # ------------------------------------------------------------------ validation
    def _validate_parameters(self) -> None:
        """awq.py:95-112 (same exception types and messages)."""
        if self.bits not in [4, 8]:
            raise ValueError(f"Unsupported bit width: {self.bits}. Supported: 4, 8.")
        if self.group_size <= 0 or not isinstance(self.group_size, int):
            raise ValueError(f"Group size must be a positive integer: {self.group_size}")
        if self.zero_point not in ["none", "minmax", "percentile"]:
            raise ValueError(f"Unsupported zero point calibration method: {self.zero_point}")
        if self.zero_point == "percentile" and (self.percentile <= 0 or self.percentile >= 1):
            raise ValueError(f"Percentile must be in range (0, 1): {self.percentile}")
        if self.scale_method not in ["minmax", "mse", "search", "awq"]:
            raise ValueError(f"Unsupported scale calibration method: {self.scale_method}")
        if self.scale_method in ("search", "awq"):
            if not isinstance(self.search_grid, int) or self.search_grid < 1:
                raise ValueError(f"search_grid must be a positive integer: {self.search_grid}")
        if self.scale_method == "awq" and self.search_grid > _hip.ACT_MAX_GRID:
            raise ValueError(f"search_grid must be <= {_hip.ACT_MAX_GRID} for scale_method='awq': {self.search_grid}")
        if self.scale_method == "search":
            if not (0 < self.search_max_shrink <= 1):
                raise ValueError(f"search_max_shrink must be in (0, 1]: {self.search_max_shrink}")

    @property
    def search_candidates(self) -> int:
        """Number of clip candidates of scale_method="search" (0 = plain RTN)."""
        if self.scale_method != "search":
            return 0
        return min(self.search_grid, max(1, int(self.search_max_shrink * self.search_grid)))

    def _search_args(self):
        """(n_grid, n_candidates) of scale_method="search" for ragged launches, else None."""
        return (self.search_grid, self.search_candidates) if self.search_candidates > 1 else None

    def _launch(self, x, rows, K, L, small: bool = False, **outs) -> None:
        if self.scale_method == "search":
            _hip.quantize_search(x, rows, K, L, self.bits, self.symmetric, self.search_grid,
                                 self.search_candidates, small=small, **outs)
        else:
            _hip.quantize_groups(x, rows, K, L, self.bits, self.symmetric, small=small, **outs)

    def _calculate_qmin_qmax(self) -> Tuple[int, int]:
        """awq.py:114-128."""
        if self.symmetric:
            return -(2 ** (self.bits - 1)), 2 ** (self.bits - 1) - 1
        return 0, 2 ** self.bits - 1

    # ------------------------------------------------------------------ helpers
    def compute_device(self) -> torch.device:
        """The GPU the kernels run on.  `self.device` keeps the reference's string
        semantics; a "cpu" quantizer still computes on the current GPU (results are
        identical and returned on the CPU), because this build has no CPU path."""
        if self.device.startswith("cuda"):
            dev = torch.device(self.device)
            if dev.index is None and torch.cuda.is_available():
                dev = torch.device("cuda", torch.cuda.current_device())
        elif torch.cuda.is_available():
            dev = torch.device("cuda", torch.cuda.current_device())
        else:
            dev = torch.device("cpu")
        _hip.require_device(dev)
        return dev

    def _check_mode(self) -> None:
        if self.zero_point == "percentile":
            # The reference's percentile branch (awq.py:187-190) calls
            # get_percentile_value(tensor, p, stats) against a 2-argument helper
            # (utils/tensor_utils.py:87) and therefore always raises this TypeError;
            # quantize_model() then skips every tensor.  Reproduced as behaviour.
            raise TypeError("get_percentile_value() takes 2 positional arguments but 3 were given")

    @staticmethod
    def _check_input(tensor) -> None:
        if not isinstance(tensor, torch.Tensor):
            raise ValueError(f"Expected torch.Tensor, got {type(tensor)}")
        if not tensor.is_floating_point():
            raise ValueError(f"Expected floating point tensor, got {tensor.dtype}")
        if tensor.dtype not in _hip.AWQ_DTYPE:
            raise RuntimeError(f"\"min_all\" not implemented for '{tensor.dtype}'")

    def _layout(self, tensor: torch.Tensor):
        """(rows, K, L, small) following awq.py:297-320 and :130-171."""
        n = tensor.numel()
        if n < self.group_size:
            if n == 0:
                raise RuntimeError("min(): Expected reduction dim to be specified for input.numel() == 0. "
                                   "Specify the reduction dim with the 'dim' argument.")
            if tensor.dim() <= 1 or not self.per_channel:
                return 1, n, n, "tensor"
            rows = tensor.shape[0]
            return rows, n // rows, n // rows, "row"
        rows, K = rows_k(tensor.shape)
        return rows, K, self.group_size, None

    # ------------------------------------------------------------------ reference API
    def quantize(self, tensor: torch.Tensor) -> Dict[str, torch.Tensor]:
        """
        Quantize a single tensor (awq.py:376-433).

        Returns a dict of CPU tensors: tensor_q (int32, input shape), scales (float16,
        [rows, groups]; 0-d or [rows] for tensors smaller than one group), zero_points
        (int32, same shape as scales), bits / group_size (int32 0-d), symmetric (bool 0-d).
        """
        return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in self._quantize_device(tensor).items()}

    def _quantize_device(self, tensor: torch.Tensor) -> Dict[str, torch.Tensor]:
        """quantize() with the result tensors left on the device."""
        self._check_input(tensor)
        rows, K, L, small = self._layout(tensor)
        self._check_mode()
        dev = self.compute_device()
        x = aligned(tensor.detach().to(dev).contiguous())
        G = groups(K, L)
        tensor_q = torch.empty(rows * K, dtype=torch.int32, device=dev)
        scales = torch.empty((rows, G), dtype=torch.float16, device=dev)
        zeros = torch.empty((rows, G), dtype=torch.int32, device=dev)
        # (small-tensor path: its scales reach fp16 straight from the input dtype, awq.py:130-171
        #  -> 411, not through the fp32 buffer of awq.py:327 — only NaN scale bits differ)
        self._launch(x, rows, K, L, small=small is not None, scales=scales, tensor_q=tensor_q, zeros=zeros)
        if small == "tensor":
            scales, zeros = scales.reshape(()), zeros.reshape(())
        elif small == "row":
            scales, zeros = scales.reshape(rows), zeros.reshape(rows)
        return {"tensor_q": tensor_q.reshape(tensor.shape), "scales": scales, "zero_points": zeros,
                **result_meta(self.bits, self.group_size, self.symmetric)}

    def quantize_model(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, Dict[str, torch.Tensor]]:
        """awq.py:435-457: quantize every tensor; failures are logged and skipped."""
        out = {}
        for name, tensor in tensors.items():
            try:
                self.logger.info(f"Quantizing tensor: {name}")
                out[name] = self.quantize(tensor)
                self.logger.info(f"Successfully quantized tensor: {name}")
            except Exception as e:  # reference semantics: skip and continue
                self.logger.error(f"Error quantizing tensor: {name}, error: {e}")
                continue
        return out

    def dequantize(self, quantized_tensor: Dict[str, torch.Tensor]) -> torch.Tensor:
        """
        awq.py:459-539: (tensor_q - zero_points) * fp16 scale, evaluated in fp16 like the
        reference, returned as float32 on the CPU.  Uses the dict's own group_size.
        """
        tq = quantized_tensor["tensor_q"]
        scales = quantized_tensor["scales"]
        zeros = quantized_tensor["zero_points"]
        L, = read_meta(quantized_tensor, "group_size")
        rows, K = rows_k(tq.shape)
        G = groups(K, L)
        if scales.dim() != 2 or zeros.dim() != 2:
            raise IndexError(f"too many indices for tensor of dimension {scales.dim()}")
        if tuple(scales.shape) != (rows, G) or tuple(zeros.shape) != (rows, G):
            raise IndexError(f"scales/zero_points shape {tuple(scales.shape)} does not match "
                             f"{rows} rows x {G} groups")
        dev = self.compute_device()
        out = torch.empty(tq.shape, dtype=torch.float32, device=dev)
        if tq.numel():
            _hip.dequantize(tq.to(dev, torch.int32).contiguous(), scales.to(dev, torch.float16).contiguous(),
                            zeros.to(dev, torch.int32).contiguous(), rows, K, L, out)
        return out.cpu()

    # ------------------------------------------------------------------ reference private methods
    # awq.py:130-374 on the HIP kernels: reference_private.py

    def _home(self, t: torch.Tensor) -> torch.Tensor:
        from . import reference_private as ref
        return ref.home(self, t)

    def _torch_gpu(self) -> bool:
        """The reference would evaluate on a GPU (self.device is a CUDA device)."""
        return self.device.startswith("cuda")

    def _on_gpu(self, tensor: torch.Tensor) -> torch.Tensor:
        from . import reference_private as ref
        return ref.on_gpu(self, tensor)

    def _compute_scale_zp_for_group(self, tensor: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """awq.py:173-213: (scale, zero_point) of the whole tensor as one group."""
        from . import reference_private as ref
        return ref.compute_scale_zp_for_group(self, tensor)

    def _calculate_scale_zp(self, tensor: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """awq.py:130-171: one group for the whole tensor, else one per dim-0 channel."""
        from . import reference_private as ref
        return ref.calculate_scale_zp(self, tensor)

    def _home_device(self) -> torch.device:
        """Where the reference's tensor.to(self.device) puts a tensor (awq.py:141, 233, 303)."""
        from . import reference_private as ref
        return ref.home_device(self)

    @staticmethod
    def _sub_check(a: torch.dtype, b: torch.dtype) -> None:
        """ATen's sub_check: `-` with a bool operand raises."""
        from . import reference_private as ref
        return ref.sub_check(a, b)

    @staticmethod
    def _param_words(p: torch.Tensor, dev: torch.device) -> Tuple[torch.Tensor, int]:
        """A parameter on the device as 8-byte words, and its kind."""
        from . import reference_private as ref
        return ref.param_words(p, dev)

    _UNSIGNED_NAMES = {torch.uint16: "UInt16", torch.uint32: "UInt32", torch.uint64: "UInt64"}

    def _apply(self, tensor: torch.Tensor, scale, zero_point, mode: int) -> torch.Tensor:
        """_quantize_tensor (mode 0) / _dequantize_tensor (mode 1) as the reference evaluates them."""
        from . import reference_private as ref
        return ref.apply(self, tensor, scale, zero_point, mode)

    def _quantize_tensor(self, tensor: torch.Tensor, scale: torch.Tensor, zero_point: torch.Tensor) -> torch.Tensor:
        """awq.py:215-250: clamp(round(tensor / scale + zero_point), qmin, qmax), a float
        tensor of the input dtype (NaN stays NaN)."""
        return self._apply(tensor, scale, zero_point, 0)

    def _dequantize_tensor(self, tensor_q: torch.Tensor, scale: torch.Tensor, zero_point: torch.Tensor) -> torch.Tensor:
        """awq.py:252-284: (tensor_q - zero_point) * scale in the tensors' dtype."""
        return self._apply(tensor_q, scale, zero_point, 1)

    def _quantize_per_group(self, tensor: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """awq.py:286-374: (tensor_q int32, scales fp32 [rows, G], zero_points fp32 [rows, G])."""
        from . import reference_private as ref
        return ref.quantize_per_group(self, tensor)

    # ------------------------------------------------------------------ packed extension
    def packed_shapes(self, shape) -> dict:
        """Shapes of the packed outputs for an input of `shape` (group path only)."""
        return packed_shapes(shape, self.group_size, self.bits)

    def quantize_packed(self, tensor: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Quantize into packed device tensors: qweight int32 [rows, ceil(K*bits/32)],
        qzeros int32 [rows, ceil(G*bits/32)], scales fp16 [rows, G] (nibble/byte j of a word
        = element j of its run of 32/bits, value q - qmin).  Values are those of quantize()."""
        self._check_input(tensor)
        self._check_mode()
        if tensor.numel() < self.group_size:
            raise ValueError("quantize_packed needs at least one full group (numel >= group_size)")
        dev = self.compute_device()
        x = aligned(tensor.detach().to(dev).contiguous())
        r = _alloc_packed(self, tensor.shape, dev)
        rows, K = rows_k(tensor.shape)
        kw = {}
        if self.search_candidates or not _hip.packs_directly(x.dtype, rows, K, self.group_size):
            kw = dict(tensor_q=torch.empty(rows * K, dtype=torch.int32, device=dev),
                      zeros=torch.empty(r["scales"].shape, dtype=torch.int32, device=dev))
        self._launch(x, rows, K, self.group_size, qweight=r["qweight"], qzeros=r["qzeros"], scales=r["scales"], **kw)
        return r

    def _packed_outputs(self, tensor: torch.Tensor) -> Dict[str, torch.Tensor]:
        """quantize_packed()'s result dict for `tensor`'s shape, outputs allocated on the
        compute device and not yet written."""
        return _alloc_packed(self, tensor.shape, self.compute_device())

    def quantize_model_packed(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, Dict[str, torch.Tensor]]:
        """Packed quantization of many tensors: the fast-path-eligible tensors (bf16, fp16 or fp32,
        group_size 32/64/128/256, K % group_size == 0) go into one ragged launch per dtype (with the
        clip search when scale_method="search"); the rest are quantized one by one.  Outputs stay
        on the device.  Failures are logged and skipped."""
        from .batch import quantize_model_batched
        return quantize_model_batched(self, tensors, packed=True)

    def quantize_model_device(self, tensors: Dict[str, torch.Tensor], packed: bool = True
                              ) -> Dict[str, Dict[str, torch.Tensor]]:
        """Many tensors at once, results left on the device: packed outputs
        (quantize_model_packed) or the reference's result dicts (quantize(), unpacked int32),
        the latter also from one ragged launch per dtype for the streaming-eligible tensors.
        Failures are logged and skipped (awq.py:453-455)."""
        from .batch import quantize_model_batched
        return quantize_model_batched(self, tensors, packed=packed)

    def quantize_layer_group(self, weights: Dict[str, torch.Tensor], activations: Optional[torch.Tensor] = None,
                             *, x_mean: Optional[torch.Tensor] = None, x_sq: Optional[torch.Tensor] = None,
                             packed: bool = True, table: Optional[torch.Tensor] = None, clip: bool = False,
                             clip_grid: int = 20, clip_max_shrink: float = 0.5, loss: str = "diag",
                             samples: Optional[torch.Tensor] = None) -> dict:
        """Activation-aware scale search + quantization of linears that read one input
        (scale_method="awq"; include/awq_hip.h awq_act_*, act_search.py).

        weights: name -> [out_features, in_features] (one dtype: bf16 / fp16 / fp32);
        activations: calibration inputs [tokens, in_features], or the per-channel statistics
        x_mean = mean |x|, x_sq = mean x^2 directly.  Each weight is quantized as
        W * diag(input_scale) (quantize_packed() result dicts if packed, else quantize()'s,
        device tensors, each with "input_scale"); the caller folds 1 / input_scale into the
        op producing x.  Returns {"results", "input_scale" fp32 [in], "ratio", "best",
        "losses" fp64 [search_grid] (the candidates' diagonal-MSE losses)}.

        clip=True adds the activation-aware clip search (awq_quantize_clip_scaled): every group's
        range is shrunk by (clip_grid - i) / clip_grid, i < min(clip_grid, max(1,
        int(clip_max_shrink * clip_grid))), and the shrink with the smallest activation-weighted
        error is kept.  Packed outputs only.  The return value gains "clip": {"loss_before",
        "loss_after" (the layer group's fp64 loss with candidate 0 / with the winners),
        "clipped_fraction" (groups whose winner is not candidate 0), "per_weight": name -> the same
        three for that weight, "best_idx": name -> the winners, int32 [rows * G] on the device}.

        loss="output" scores the same candidates (the table still comes from the statistics) by
        AWQ's published objective, the layer group's output error on token samples
        sum_j ||(Q(W_j s) / s - W_j) X^T||^2 (awq_output_error; samples [tokens, in_features],
        default: `activations`), instead of its diagonal form: every candidate of every weight
        is quantized into a reused packed buffer and measured.  Same selection rule (first
        minimum, a NaN loss never wins).  The return value gains "loss": "output", "losses" are
        the output-space losses, and "diag_losses" / "diag_best" say what the diagonal search
        would have chosen.  clip=True composes with it; the clip search keeps its x_sq-weighted
        (diagonal) loss.  loss="diag" (default) is the search described above, unchanged."""
        from .act_search import quantize_layer_group
        return quantize_layer_group(self, weights, activations, x_mean=x_mean, x_sq=x_sq, packed=packed, table=table,
                                    clip=clip, clip_grid=clip_grid, clip_max_shrink=clip_max_shrink, loss=loss,
                                    samples=samples)

    def _output_search(self, sr: dict, samples: torch.Tensor) -> dict:
        """quantize_layer_group's loss="output" (act_search.output_search)."""
        from .act_search import output_search
        return output_search(self, sr, samples)

    def _clip_layer_group(self, weights, sr: dict, clip_grid: int, n_clip: int) -> dict:
        """quantize_layer_group's last step with clip=True (act_search.clip_layer_group)."""
        from .act_search import clip_layer_group
        return clip_layer_group(self, weights, sr, clip_grid, n_clip)

    def quantize_block(self, tensors: Dict[str, torch.Tensor], stats: Dict[str, Tuple[torch.Tensor, torch.Tensor]],
                       block, *, clip: bool = False, clip_grid: int = 20, clip_max_shrink: float = 0.5,
                       samples: Optional[Dict[str, torch.Tensor]] = None, loss: str = "diag") -> dict:
        """Activation-aware quantization of one decoder block with the searched input scales
        folded into the ops that produce each input (block_plan.Block; scale_method="awq").

        tensors: name -> tensor of the block's members and producers (block.tensor_names());
        stats: name -> (x_mean, x_sq) as load_act_stats returns.  A group's statistics are those
        of its first member, in table order, that has any; other members' statistics that differ
        are reported with a warning and ignored.

        Order (fixed):
          1. attn_out and mlp_out: one quantize_layer_group call on the single member each
             (clip=True applies to that call), yielding s_out;
          2. each s_out folded into its producer's rows (v_proj / up_proj, a device copy) and
             bias with awq_fold_rows;
          3. attn_in on {q, k, v_folded} and mlp_in on {gate, up_folded}: one joint
             quantize_layer_group call each, yielding s_in;
          4. each s_in folded into its norm weight with awq_fold_rows (K = 1).
        So the v_proj / up_proj that is searched and quantized is the one the checkpoint holds.
        (AutoAWQ folds the rows after the attn_in search; parity with AutoAWQ is unpinned.)

        A group that is not folded (not foldable — e.g. attn_out with grouped-query shapes — or
        without statistics) keeps s = 1: its members take quantize_packed, or with clip=True and
        statistics quantize_layer_group(table=ones [search_grid, in], clip=True), so the clip
        search still weighs by x_sq.

        Returns device tensors: {"results": name -> quantize_packed()-style dict (no
        "input_scale": the fold is done), "folded": name -> folded norm weight / bias,
        "scales": {"<weight>.input_scale": s fp32 [in] for every member, "<weight>.row_scale":
        fp32 [out] for every row-folded producer}, "groups": group -> {"ratio", "losses",
        "folded", "clip"}}.

        loss="output" (quantize_layer_group's) with samples: group name (attn_in, attn_out, mlp_in,
        mlp_out) -> token samples [tokens, in] of that group's input, passed to the four calls in
        the order above.  The samples are the UNFOLDED inputs (what the calibration forward saw):
        the search's col_scale already accounts for the fold.  A folded group without samples
        falls back to the diagonal loss with a warning.  Such groups' reports gain "loss", "best"
        and "diag_best"."""
        from .act_search import quantize_block
        return quantize_block(self, tensors, stats, block, clip=clip, clip_grid=clip_grid,
                              clip_max_shrink=clip_max_shrink, samples=samples, loss=loss)

    def export_autoawq(self, packed: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """A quantize_packed() result of a 2-D [out_features, in_features] weight in the
        AutoAWQ "GEMM" layout (include/awq_hip.h awq_export_autoawq_gemm): qweight int32
        [in, out/8], qzeros int32 [in/group_size, out/8], scales fp16 [in/group_size, out],
        packed along out_features with AWQ_ORDER.  Device tensors; 4-bit only."""
        from .autoawq import export_autoawq
        return export_autoawq(self, packed)

    def import_autoawq(self, gemm: Dict[str, torch.Tensor], group_size: Optional[int] = None,
                       symmetric: Optional[bool] = None) -> Dict[str, torch.Tensor]:
        """The inverse of export_autoawq (include/awq_hip.h awq_import_autoawq_gemm): `gemm` holds
        qweight int32 [in, out/8], qzeros int32 [in/group_size, out/8] and scales fp16
        [in/group_size, out] of one linear in the AutoAWQ "GEMM" layout, on the CPU or the
        device.  Returns a quantize_packed()-shaped dict on the device (row-major qweight /
        qzeros / scales, bits = 4, group_size and symmetric — defaults: the quantizer's —
        and shape = [out, in]) that dequantize_packed, quantization_error and export_autoawq
        take unchanged.  ValueError for inconsistent shapes, RuntimeError for what the C call
        refuses."""
        from .autoawq import import_autoawq
        return import_autoawq(self, gemm, group_size, symmetric)

    def dequantize_autoawq(self, gemm: Dict[str, torch.Tensor], group_size: Optional[int] = None,
                           symmetric: Optional[bool] = None, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """import_autoawq, then dequantize_packed: the [out, in] weight a GEMM-layout linear holds."""
        from .autoawq import dequantize_autoawq
        return dequantize_autoawq(self, gemm, group_size, symmetric, dtype)

    def export_gptq(self, packed, checkpoint_format: str = "gptq") -> Dict[str, torch.Tensor]:
        """A 2-D [out_features, in_features] weight in AutoGPTQ's 4-bit layout, desc_act = false
        (include/awq_hip.h awq_export_gptq): `packed` is a quantize_packed() result, or the weight
        itself (it is then quantized first).  qweight int32 [in/8, out] (nibble i of word (r, n) =
        element 8r + i of row n), qzeros int32 [in/group_size, out/8], scales fp16
        [in/group_size, out], g_idx int32 [in] = k // group_size; sequential nibbles, no
        interleave.  Symmetric results keep their fields (q + 8, zero 8).  checkpoint_format
        "gptq" (v1) stores zero - 1 modulo 16, "gptq_v2" the zero itself; "zero_points_at_0"
        (int64 0-d, on the device) counts the zero points v1 stores as 15.  Device tensors."""
        from .gptq import export_gptq
        if isinstance(packed, torch.Tensor):
            packed = self.quantize_packed(packed)
        return export_gptq(self, packed, checkpoint_format)

    def import_gptq(self, gptq: Dict[str, torch.Tensor], group_size: Optional[int] = None,
                    symmetric: Optional[bool] = None, checkpoint_format: str = "gptq") -> Dict[str, torch.Tensor]:
        """The inverse of export_gptq (include/awq_hip.h awq_import_gptq): `gptq` holds qweight,
        qzeros and scales of one linear in the GPTQ layout (and optionally g_idx, which must be
        k // group_size: act-order is not supported), on the CPU or the device.  Returns a
        quantize_packed()-shaped dict on the device, as import_autoawq does.  ValueError for
        inconsistent shapes, an unknown checkpoint_format or an act-order g_idx; RuntimeError for
        what the C call refuses."""
        from .gptq import import_gptq
        return import_gptq(self, gptq, group_size, symmetric, checkpoint_format)

    def dequantize_gptq(self, gptq: Dict[str, torch.Tensor], group_size: Optional[int] = None,
                        symmetric: Optional[bool] = None, checkpoint_format: str = "gptq",
                        dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """import_gptq, then dequantize_packed: the [out, in] weight a GPTQ-layout linear holds."""
        from .gptq import dequantize_gptq
        return dequantize_gptq(self, gptq, group_size, symmetric, checkpoint_format, dtype)

    def quantize_gptq(self, tensor: torch.Tensor, samples: Optional[torch.Tensor] = None, *,
                      hessian: Optional[torch.Tensor] = None, input_scale: Optional[torch.Tensor] = None,
                      damp: float = 0.01) -> Dict[str, torch.Tensor]:
        """quantize_packed with GPTQ's error-compensated rounding instead of round-to-nearest
        (gptq_round.py; include/awq_hip.h awq_gptq_round_block): a 2-D
        [out_features, in_features] bf16 / fp16 / fp32 weight, group_size 32 / 64 / 128 dividing
        in_features, static groups (no act-order).

        samples [tokens, in_features]: token samples of the linear's input; H = X^T X is formed
        from them in fp32 on the device.  hessian [in, in] replaces it (samples are then only
        used for the report).  A column with H[c][c] == 0 gets H[c][c] = 1 and its working weight
        zeroed; damp * mean(diag H) is added to the diagonal; U = cholesky(cholesky_inverse(
        cholesky(H)), upper) (torch.linalg on the device).  Blocks of 128 columns: the kernel,
        then one GEMM takes the block's errors off the columns to its right.
        input_scale s fp32 [in] (quantize_layer_group's): the weight is W * diag(s)
        (awq_apply_input_scale) and the samples X * diag(RN(1 / s)).

        Returns the quantize_packed() dict (device tensors; "input_scale" when one was given) plus
        "rounding": {"loss", "loss_rtn": the output error sum ((W^ - W) X^T)^2 of the result and of
        round-to-nearest on the samples (awq_output_error, in the original domain; None without
        samples), "dead_columns", "damp" (the value used), "fallback"}.  A failed factorisation
        multiplies damp by 10, three tries in all; after that, and for a non-finite weight or
        Hessian, the result is quantize_packed's, with a warning and fallback = True."""
        from .gptq_round import quantize_gptq
        return quantize_gptq(self, tensor, samples, hessian=hessian, input_scale=input_scale, damp=damp)

    def dequantize_packed(self, packed: Dict[str, torch.Tensor], dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """Inverse of quantize_packed with the reference's dequantize arithmetic (fp16 math)."""
        from .autoawq import dequantize_packed
        return dequantize_packed(self, packed, dtype)

    # ------------------------------------------------------------------ quantization-error report
    def quantization_error(self, tensor: torch.Tensor, result: Dict[str, torch.Tensor],
                           per_group: bool = False, samples: Optional[torch.Tensor] = None) -> dict:
        """What `result` costs against the original `tensor`: the reference's only quality figure
        (torch.abs(tensor - dequantized).mean(), its test_quantization.py:155-160) and its
        relatives, from one pass over the weights and the PACKED result (include/awq_hip.h
        awq_quant_error) — so it measures any scale method and any checkpoint this tool wrote.

        result: a quantize_packed() dict, or a reference-format dict (tensor_q / scales /
        zero_points; packed on the device with its own bits / symmetric).  Shape, bits and group
        size are the dict's.  Like dequantize(), 0-d or 1-d scales (small-tensor results) raise
        IndexError.  Returns plain Python numbers: numel, nonfinite (elements whose error, its
        square or w^2 is NaN / inf: they enter no sum), sum_abs, sum_sq, sum_w_sq,
        mean_abs_error = sum_abs / (numel - nonfinite) (NaN when nothing is finite), mse,
        max_abs_error, snr_db = 10 log10(sum_w_sq / sum_sq) (inf when sum_sq == 0).
        A result of quantize_layer_group / --act_stats carries "input_scale" and quantizes
        W * diag(input_scale) (the caller folds 1 / input_scale into the op producing x): the
        report is then taken against RN(W * input_scale) in the weight dtype (awq_apply_input_scale),
        i.e. in the scaled domain the checkpoint lives in, and "input_scaled" is True.
        per_group=True adds the device tensors group_abs / group_sq / group_w_sq / group_max (fp32
        [rows, G]) and group_nonfinite (int32 [rows, G]).

        samples [tokens, in_features] (CPU or device, converted to the weight's dtype) adds what the
        result costs at the linear's OUTPUT on those inputs (include/awq_hip.h awq_output_error):
        output_sum_sq = sum (W^ x - W x)^2 and output_ref_sq = sum (W x)^2 over rows and tokens (the
        fp32 per-row sums added in fp64), output_rel_error = sqrt(output_sum_sq / output_ref_sq),
        output_snr_db, output_tokens; per_group=True also the device tensors row_output_sq /
        row_output_ref_sq (fp32 [rows]).  For a result that carries input_scale these are taken in
        the ORIGINAL domain — the original tensor, w^ = dq / input_scale, unscaled samples: the
        layer as the model runs it after the fold — while the weight-space figures above stay in
        the scaled domain.  A shape mismatch raises ValueError before any device work."""
        from .report import quantization_error
        return quantization_error(self, tensor, result, per_group, samples)

    def quantization_error_model(self, tensors: Dict[str, torch.Tensor],
                                 results: Dict[str, Dict[str, torch.Tensor]]) -> Dict[str, dict]:
        """quantization_error for every result; failures (and results without a source tensor)
        are logged and skipped, like quantize_model."""
        from .report import quantization_error_model
        return quantization_error_model(self, tensors, results)


def _alloc_packed(q: AWQQuantizer, shape, dev: torch.device) -> Dict[str, torch.Tensor]:
    """quantize_packed()'s result dict for an input of `shape`: unwritten outputs on `dev`, and the metadata."""
    sh = q.packed_shapes(tuple(shape))
    return {"qweight": torch.empty(sh["qweight"], dtype=torch.int32, device=dev),
            "qzeros": torch.empty(sh["qzeros"], dtype=torch.int32, device=dev),
            "scales": torch.empty(sh["scales"], dtype=torch.float16, device=dev),
            **result_meta(q.bits, q.group_size, q.symmetric, shape)}
