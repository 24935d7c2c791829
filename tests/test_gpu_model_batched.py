"""quantize_model_packed and quantize_model_device(packed=False) on one mixed set of tensors:
which tensors come back and in what order, every returned tensor bit for bit what
quantize_packed / quantize gives for that tensor alone, and the exact ERROR records.

The two entry points share one routine (quantization/batch.py quantize_model_batched) and
differ on purpose: the packed one refuses tensors below one group and raises for
zero_point="percentile", the unpacked one sends the former through quantize()'s small-tensor
path and logs the latter per tensor like the reference's quantize_model.  The expectations
were recorded from the two separate routines this one replaced.
"""
import logging

import pytest
import torch

pytestmark = pytest.mark.gpu

GS = 128
PERCENTILE_ERROR = "get_percentile_value() takes 2 positional arguments but 3 were given"
REFUSED = {"h_int32": "Expected floating point tensor, got torch.int32",
           "i_list": "Expected torch.Tensor, got <class 'list'>"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from awq_quantizer import _hip
    _hip.require_device(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def tensors():
    g = torch.Generator().manual_seed(1234)
    rand = lambda shape, dtype: (torch.randn(*shape, generator=g) * 0.02).to(dtype)
    flat = rand((4 * 256 + 8,), torch.bfloat16).to("cuda")
    view = flat[1:1 + 4 * 256].view(4, 256)          # contiguous, base 2 bytes past a 16-B boundary
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return {"a_bf16": rand((4, 256), torch.bfloat16),
            "b_bf16": rand((8, 128), torch.bfloat16),
            "c_f16": rand((4, 256), torch.float16),
            "d_f32": rand((2, 384), torch.float32),
            "e_f64": rand((2, 256), torch.float64),
            "f_tail": rand((3, 100), torch.bfloat16),     # K is no multiple of the group size
            "g_small": rand((64,), torch.bfloat16),       # numel below the group size
            "h_int32": torch.arange(256, dtype=torch.int32).reshape(2, 128),
            "i_list": [0.5] * 256,
            "j_view": view}


def quantizer(name, **kw):
    """An AWQQuantizer and the list its ERROR records' messages are appended to."""
    from awq_quantizer.quantization import AWQQuantizer
    q = AWQQuantizer(bits=4, group_size=GS, symmetric=False, device="cuda:0", logger_name=name,
                     logger_level="ERROR", **kw)
    records = []

    class Collect(logging.Handler):
        def emit(self, record):
            records.append((record.levelname, record.getMessage()))

    logging.getLogger(name).addHandler(Collect(level=logging.ERROR))
    return q, records


def same(got, want, name):
    assert sorted(got) == sorted(want), name      # (a batch's dict lists scales first)
    for k in want:
        g, w = got[k].cpu(), want[k].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k)
        if g.dtype == torch.float16:
            g, w = g.view(torch.int16), w.view(torch.int16)
        assert torch.equal(g, w), (name, k)


def errors(names_and_messages):
    return [("ERROR", f"Error quantizing tensor: {n}, error: {m}") for n, m in names_and_messages]


@pytest.mark.parametrize("scale_method", ["mse", "search"])
def test_packed(tensors, scale_method):
    q, records = quantizer(f"batched_packed_{scale_method}", scale_method=scale_method)
    out = q.quantize_model_packed(tensors)
    assert list(out) == ["a_bf16", "b_bf16", "c_f16", "d_f32", "e_f64", "f_tail", "j_view"]
    assert records == errors([("g_small", "numel < group_size"), ("h_int32", REFUSED["h_int32"]),
                              ("i_list", REFUSED["i_list"])])
    for name, res in out.items():
        assert res["qweight"].is_cuda
        same(res, q.quantize_packed(tensors[name]), name)
    again = q.quantize_model_device(tensors)          # packed=True is the same call
    assert list(again) == list(out)
    for name in out:
        same(again[name], out[name], name)


@pytest.mark.parametrize("scale_method", ["mse", "search"])
def test_unpacked(tensors, scale_method):
    q, records = quantizer(f"batched_unpacked_{scale_method}", scale_method=scale_method)
    out = q.quantize_model_device(tensors, packed=False)
    assert list(out) == ["a_bf16", "b_bf16", "c_f16", "d_f32", "e_f64", "f_tail", "g_small", "j_view"]
    assert records == errors([("h_int32", REFUSED["h_int32"]), ("i_list", REFUSED["i_list"])])
    for name, res in out.items():
        assert res["tensor_q"].is_cuda
        same(res, q.quantize(tensors[name]), name)


def test_percentile(tensors):
    q, records = quantizer("batched_percentile", zero_point="percentile", percentile=0.99)
    with pytest.raises(TypeError, match="get_percentile_value"):
        q.quantize_model_packed(tensors)
    assert records == []
    assert q.quantize_model_device(tensors, packed=False) == {}
    assert records == errors([(n, REFUSED.get(n, PERCENTILE_ERROR)) for n in tensors])
