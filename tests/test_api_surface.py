"""AWQQuantizer's surface after quantization/awq.py was split into modules: every attribute the
class had before the split is still there, every callable has the same signature, and the
docstrings users read on the class and its public methods are unchanged.

API is the class before the split (commit 211489d): (name, kind of the class attribute,
str(inspect.signature(...)), first 16 hex digits of the SHA-256 of __doc__ for the class and its
public methods).  A deliberate API change edits the row it touches.
"""
import hashlib
import inspect

import pytest

API = [
    ('__doc__', 'str', None, '600e5a9a8a43003e'),
    ('__init__', 'function',
     "(self, bits: int = 4, group_size: int = 128, symmetric: bool = True, zero_point: str = 'minmax', percentile: float = 0.99, scale_method: str = 'mse', per_channel: bool = True, device: Optional[str] = None, logger_name: str = 'awq_quantizer', logger_level: str = 'INFO', logger_to_file: bool = False, logger_file_path: Optional[str] = None, search_grid: int = 20, search_max_shrink: float = 0.5, duo_scaling: bool = True)",
     None),
    ('_validate_parameters', 'function', '(self) -> None', None),
    ('search_candidates', 'property', '(self) -> int', 'b5d96f348948e82b'),
    ('_search_args', 'function', '(self)', None),
    ('_launch', 'function', '(self, x, rows, K, L, small: bool = False, **outs) -> None', None),
    ('_calculate_qmin_qmax', 'function', '(self) -> Tuple[int, int]', None),
    ('compute_device', 'function', '(self) -> torch.device', 'f0b0341536fdb95a'),
    ('_check_mode', 'function', '(self) -> None', None),
    ('_check_input', 'staticmethod', '(tensor) -> None', None),
    ('_layout', 'function', '(self, tensor: torch.Tensor)', None),
    ('quantize', 'function', '(self, tensor: torch.Tensor) -> Dict[str, torch.Tensor]', '6422207bd066c653'),
    ('_quantize_device', 'function', '(self, tensor: torch.Tensor) -> Dict[str, torch.Tensor]', None),
    ('quantize_model', 'function',
     '(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, Dict[str, torch.Tensor]]',
     'c12582d229120703'),
    ('dequantize', 'function',
     '(self, quantized_tensor: Dict[str, torch.Tensor]) -> torch.Tensor',
     '0867821776ddfe46'),
    ('_home', 'function', '(self, t: torch.Tensor) -> torch.Tensor', None),
    ('_torch_gpu', 'function', '(self) -> bool', None),
    ('_on_gpu', 'function', '(self, tensor: torch.Tensor) -> torch.Tensor', None),
    ('_compute_scale_zp_for_group', 'function',
     '(self, tensor: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]',
     None),
    ('_calculate_scale_zp', 'function', '(self, tensor: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]', None),
    ('_home_device', 'function', '(self) -> torch.device', None),
    ('_sub_check', 'staticmethod', '(a: torch.dtype, b: torch.dtype) -> None', None),
    ('_param_words', 'staticmethod', '(p: torch.Tensor, dev: torch.device) -> Tuple[torch.Tensor, int]', None),
    ('_UNSIGNED_NAMES', 'dict', None, None),
    ('_apply', 'function', '(self, tensor: torch.Tensor, scale, zero_point, mode: int) -> torch.Tensor', None),
    ('_quantize_tensor', 'function',
     '(self, tensor: torch.Tensor, scale: torch.Tensor, zero_point: torch.Tensor) -> torch.Tensor',
     None),
    ('_dequantize_tensor', 'function',
     '(self, tensor_q: torch.Tensor, scale: torch.Tensor, zero_point: torch.Tensor) -> torch.Tensor',
     None),
    ('_quantize_per_group', 'function',
     '(self, tensor: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]',
     None),
    ('packed_shapes', 'function', '(self, shape) -> dict', '10710487eeda5f4b'),
    ('quantize_packed', 'function', '(self, tensor: torch.Tensor) -> Dict[str, torch.Tensor]', '4acb115275dd6487'),
    ('_packed_outputs', 'function', '(self, tensor: torch.Tensor) -> Dict[str, torch.Tensor]', None),
    ('quantize_model_packed', 'function',
     '(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, Dict[str, torch.Tensor]]',
     'fe8caab143181abc'),
    ('quantize_model_device', 'function',
     '(self, tensors: Dict[str, torch.Tensor], packed: bool = True) -> Dict[str, Dict[str, torch.Tensor]]',
     '892caaeaa32e3c54'),
    ('quantize_layer_group', 'function',
     "(self, weights: Dict[str, torch.Tensor], activations: Optional[torch.Tensor] = None, *, x_mean: Optional[torch.Tensor] = None, x_sq: Optional[torch.Tensor] = None, packed: bool = True, table: Optional[torch.Tensor] = None, clip: bool = False, clip_grid: int = 20, clip_max_shrink: float = 0.5, loss: str = 'diag', samples: Optional[torch.Tensor] = None) -> dict",
     'b2f75e295c31bd73'),
    ('_output_search', 'function', '(self, sr: dict, samples: torch.Tensor) -> dict', None),
    ('_clip_layer_group', 'function', '(self, weights, sr: dict, clip_grid: int, n_clip: int) -> dict', None),
    ('quantize_block', 'function',
     "(self, tensors: Dict[str, torch.Tensor], stats: Dict[str, Tuple[torch.Tensor, torch.Tensor]], block, *, clip: bool = False, clip_grid: int = 20, clip_max_shrink: float = 0.5, samples: Optional[Dict[str, torch.Tensor]] = None, loss: str = 'diag') -> dict",
     '57618814861c7351'),
    ('export_autoawq', 'function',
     '(self, packed: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]',
     '452d43e682c57597'),
    ('import_autoawq', 'function',
     '(self, gemm: Dict[str, torch.Tensor], group_size: Optional[int] = None, symmetric: Optional[bool] = None) -> Dict[str, torch.Tensor]',
     '3ec0f018dddef6b8'),
    ('dequantize_autoawq', 'function',
     '(self, gemm: Dict[str, torch.Tensor], group_size: Optional[int] = None, symmetric: Optional[bool] = None, dtype: torch.dtype = torch.float32) -> torch.Tensor',
     'f6ef2b3d025a0155'),
    ('dequantize_packed', 'function',
     '(self, packed: Dict[str, torch.Tensor], dtype: torch.dtype = torch.float32) -> torch.Tensor',
     '72973b70c68a67ab'),
    ('quantization_error', 'function',
     '(self, tensor: torch.Tensor, result: Dict[str, torch.Tensor], per_group: bool = False, samples: Optional[torch.Tensor] = None) -> dict',
     '9852d7826e0e5152'),
    ('quantization_error_model', 'function',
     '(self, tensors: Dict[str, torch.Tensor], results: Dict[str, Dict[str, torch.Tensor]]) -> Dict[str, dict]',
     '1f8adce4a76a1c7f'),
]


def _function(v):
    return v.__func__ if isinstance(v, staticmethod) else (v.fget if isinstance(v, property) else v)


@pytest.mark.parametrize("name,kind,signature,doc", API, ids=[row[0] for row in API])
def test_attribute_is_unchanged(name, kind, signature, doc):
    from awq_quantizer.quantization.awq import AWQQuantizer
    assert name in vars(AWQQuantizer), f"AWQQuantizer.{name} is gone"
    v = vars(AWQQuantizer)[name]
    assert type(v).__name__ == kind
    f = _function(v)
    if signature is not None:
        assert str(inspect.signature(f)) == signature
    if doc is not None:
        text = v if name == "__doc__" else f.__doc__
        assert isinstance(text, str) and hashlib.sha256(text.encode()).hexdigest()[:16] == doc, \
            f"AWQQuantizer.{name}.__doc__ changed"


def test_report_functions_are_importable_from_awq():
    from awq_quantizer.quantization import report
    from awq_quantizer.quantization.awq import error_report, output_report
    assert error_report is report.error_report and output_report is report.output_report
