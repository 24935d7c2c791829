"""--output_format mxfp4: every linear weight the checkpoint formats convert, with
in_features % 32 == 0, as OCP microscaling FP4; every other tensor copied.  One process, one device,
tensor by tensor through AWQQuantizer.quantize_mxfp4 (the native streaming pipeline does not know the
format).  The directory: model.safetensors with `<prefix>.weight` (uint8 [N, K / 2]) and
`<prefix>.weight_scale` (uint8 [N, K / 32]) per converted linear, and config.json with a
`quantization_config` (output.write_mxfp4_config)."""
import time
from typing import List

from .model_loading import TensorInfo
from .output import TIMINGS, finish_run, model_type_of, save_mxfp4
from .quantization.linear_weights import CONV1D_MODEL_TYPES, is_linear_weight
from .quantization.mxfp4 import BLOCK


def main_mxfp4(args, loader, index: List[TensorInfo], ordered: List[TensorInfo], device: str, logger,
               start: float) -> int:
    from .quantization.awq import AWQQuantizer
    mtype = model_type_of(loader)
    if mtype in CONV1D_MODEL_TYPES:
        logger.warning(f"model_type {mtype}: Conv1D projection weights ([in, out]) are copied unquantized")
    linear = [i for i in ordered if is_linear_weight(i, BLOCK, mtype)]
    names = {i.name for i in linear}
    passthrough = [i for i in index if i.name not in names]
    rule = args.mxfp4_scale or "floor"
    logger.info(f"MXFP4 export (scale rule {rule}): {len(linear)} linear weights quantized, {len(passthrough)} copied")
    q = AWQQuantizer(device=device, logger_name="awq_mxfp4_quantizer", logger_level=args.log_level)
    quantized, failed = {}, []
    for info in linear:
        try:
            r = q.quantize_mxfp4(loader.read(info), rule)
            quantized[info.name] = {"codes": r["codes"].cpu(), "scales": r["scales"].cpu()}
        except Exception as e:  # noqa: BLE001  (skip and copy, like the other checkpoint formats)
            logger.error(f"Error quantizing tensor: {info.name}, error: {e}")
            failed.append(info)
    TIMINGS["quantize_s"] = time.time() - start
    return finish_run(args, linear, quantized, logger, start,
                      lambda: save_mxfp4(quantized, loader, passthrough, args.output_dir, rule, logger, failed))
