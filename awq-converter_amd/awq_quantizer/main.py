"""
awq_quantizer command line — drop-in for the reference CLI (src/awq_quantizer/main.py).

Same flags and defaults (reference main.py:22-159), same tensor filter (floating point,
numel >= 128, main.py:244-253), same processing / output order (bytes descending,
stable, main.py:259), same output layout (model_chunk_NNNN.pt holding nested result
dicts + metadata.json, main.py:430-512) and exit codes (0 ok; 1 on load failure, no
tensor quantized, or save failure).

What changes underneath, MI355X-first:
  * weights are streamed: headers are read first, then batches of tensors are read by
    reader threads into pinned host memory, copied to the GPU on a copy stream while the
    previous batch is quantized (one ragged launch per batch), and the results copied
    back asynchronously (the reference loads every file whole, then copies every tensor
    to the device eagerly, main.py:296-307, and quantizes tensor by tensor);
  * --multi_gpu / --device all really shards: the tensor list is LPT-partitioned over
    the GPUs (the reference's own partition_tensors, main.py:395-427, which it never
    calls; instead every device re-quantizes every tensor, main.py:596-606), one host
    thread per GPU;
  * the arithmetic is the HIP kernels behind include/awq_hip.h;
  * --save_safetensors works (the reference passes nested dicts to save_file and
    always fails, main.py:488-490): result dicts are flattened to "<name>.<field>";
  * --output_format packed writes qweight/qzeros/scales (int4/int8 packed) instead of
    the reference's unpacked int32 tensor_q (8x smaller on disk at 4 bits).

This module is main() and the single-process run.  The flags and their rules are options.py,
one device's quantize loop pipeline.py, every writer output.py; the --fold_scales and torchrun
runs (fold_cli.py, dist_cli.py) are imported when main() dispatches to them.
"""

import logging
import os
import sys
import threading
import time
from typing import Dict, List, Optional, Tuple

_T_MODULE = time.time()
if __name__ == "__main__":
    # the program itself (`python -m awq_quantizer.main`): HIP's first-use work starts on a
    # native thread now and overlaps `import torch` (~1.5 s); see _early.py
    from awq_quantizer import _early
    _early.start(sys.argv[1:])

import torch

_IMPORT_TORCH_S = time.time() - _T_MODULE

from .stream import device_name, start_warmup
from .model_loading import TensorInfo, load_model_from_hub
from .quantization.linear_weights import CONV1D_MODEL_TYPES, is_linear_weight
from .utils.logger import get_logger
from .options import (AUTOAWQ_NEEDS_4_BITS, CHECKPOINT_FORMATS, GPTQ_NEEDS_4_BITS, act_clip_of, check_args,
                      check_flags, parse_args, wants_samples)
from .output import ChunkWriter, _NullSink, finish_run, model_type_of, save_autoawq, writer_threads
from .pipeline import STREAM_OPTS, TIMINGS, StreamSettings, _device_worker, new_quantizer
# names that callers outside the package import from here
from .options import build_parser  # noqa: F401
from .output import (_rank_stem, _write_chunk, _write_metadata, cpu_share, run_metrics,  # noqa: F401
                     save_model_in_chunks, write_autoawq_configs)
from .pipeline import _batch_budget, _batches, quantize_stream, quantize_stream_native  # noqa: F401


def get_available_gpus(logger=None) -> List[str]:
    """["cuda:0", ...] for every visible GPU (reference main.py:162-186)."""
    if not torch.cuda.is_available():
        if logger:
            logger.warning("No CUDA devices available")
        return []
    devs = []
    for i in range(torch.cuda.device_count()):
        if logger:
            logger.info(f"Found CUDA device {i}: {device_name(i)}")
        devs.append(f"cuda:{i}")
    return devs


def get_device_memory_info(device_idx: int) -> Tuple[float, float]:
    """(total GB, free GB) of a device (reference main.py:189-213)."""
    if not torch.cuda.is_available():
        return 0.0, 0.0
    try:
        free, total = torch.cuda.mem_get_info(device_idx)
        return total / 1024 ** 3, free / 1024 ** 3
    except Exception:  # noqa: BLE001
        return 0.0, 0.0


def select_tensors(index: List[TensorInfo], logger=None) -> List[TensorInfo]:
    """Filter + order of reference main.py:241-259, on header information only."""
    keep = []
    for info in index:
        if info.dtype is None or not info.dtype.is_floating_point or info.numel == 0:
            if logger:
                logger.warning(f"Skipping invalid tensor: {info.name}")
            continue
        if info.numel < 128:
            if logger:
                logger.warning(f"Skipping tensor too small for grouping: {info.name}")
            continue
        keep.append(info)
    keep.sort(key=lambda i: i.nbytes, reverse=True)   # stable
    return keep


def prepare_tensors_for_quantization(tensors: Dict[str, torch.Tensor], device: str, max_memory_fraction: float = 0.8,
                                     batch_size: int = 10, logger=None) -> List[Dict[str, torch.Tensor]]:
    """In-memory API of reference main.py:216-330: filtered, size-ordered batches of at most
    batch_size tensors.  Tensors stay where they are (they are moved to the GPU one at a
    time when quantized, not all at once)."""
    infos = []
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            if logger:
                logger.warning(f"Skipping invalid tensor: {name}")
            continue
        infos.append(TensorInfo(name, None, t.dtype, t.shape))
    ordered = select_tensors(infos, logger)
    batches, cur = [], {}
    for info in ordered:
        if len(cur) >= batch_size:
            batches.append(cur)
            cur = {}
        cur[info.name] = tensors[info.name]
    if cur:
        batches.append(cur)
    if logger:
        logger.info(f"Created {len(batches)} batches with {sum(len(b) for b in batches)} total tensors")
    return batches


def partition_tensors(items, num_partitions: int):
    """Greedy LPT by bytes (reference main.py:395-427).  `items` is a dict name->tensor or a
    list of TensorInfo; returns num_partitions collections of the same kind."""
    if num_partitions <= 1:
        return [items]
    if isinstance(items, dict):
        sizes = [(n, t.numel() * t.element_size()) for n, t in items.items()]
    else:
        sizes = [(i, i.nbytes) for i in items]
    sizes.sort(key=lambda x: x[1], reverse=True)
    parts = [dict() if isinstance(items, dict) else [] for _ in range(num_partitions)]
    load = [0] * num_partitions
    for key, size in sizes:
        k = load.index(min(load))
        if isinstance(items, dict):
            parts[k][key] = items[key]
        else:
            parts[k].append(key)
        load[k] += size
    return parts


def load_act_stats(path: str, logger=None) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """--act_stats: '<weight name>.x_mean' / '<weight name>.x_sq' fp32 vectors (safetensors)."""
    from safetensors.torch import load_file
    flat = load_file(path)
    out = {}
    for key, t in flat.items():
        if key.endswith(".x_mean"):
            name = key[: -len(".x_mean")]
            sq = flat.get(name + ".x_sq")
            if sq is None:
                raise ValueError(f"--act_stats: {key} has no matching {name}.x_sq")
            out[name] = (t.float().reshape(-1), sq.float().reshape(-1))
    if logger:
        logger.info(f"Loaded activation statistics for {len(out)} weights from {path}")
    return out


def calibrate_for_main(args, device: str, logger,
                       samples_out: Optional[Dict[str, torch.Tensor]] = None
                       ) -> Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor]]]:
    """--calib_ids: the statistics load_act_stats would read, from a calibration forward on `device`
    (awq_quantizer/calibration); None after logging why not.  samples_out (--search_loss output):
    a dict the forward fills with --n_sample_tokens token samples per linear input."""
    from .calibration import calibrate_model, read_input_ids
    try:
        ids = read_input_ids(args.calib_ids)
        t0 = time.time()
        stats = calibrate_model(args.model_id, ids, device=device, logger=logger, samples_out=samples_out,
                                n_sample_tokens=args.n_sample_tokens if samples_out is not None else 0)
    except Exception as e:  # noqa: BLE001
        logger.error(f"--calib_ids: calibration failed: {e}")
        return None
    logger.info(f"Calibrated {len(stats)} weights on {ids.numel()} tokens in {time.time() - t0:.2f} seconds")
    return stats


def _pick_devices(args, logger) -> List[str]:
    """The devices this process drives (--device / --multi_gpu), each one logged."""
    if args.multi_gpu or args.device.lower() == "all":
        devices = get_available_gpus(logger)
        if not devices:
            logger.warning("No CUDA devices available, falling back to CPU")
            devices = ["cpu"]
        else:
            logger.info(f"Using {len(devices)} GPU(s) for processing")
    else:
        devices = [args.device]
    for d in list(devices):
        if d.startswith("cuda") and torch.cuda.is_available():
            idx = int(d.split(":")[1]) if ":" in d else 0
            total, free = get_device_memory_info(idx)
            logger.info(f"Using GPU {d}: {device_name(idx)}")
            logger.info(f"  Total memory: {total:.2f} GB")
            logger.info(f"  Free memory: {free:.2f} GB")
        elif d.startswith("cuda"):
            logger.warning(f"CUDA device {d} requested but not available, falling back to CPU")
            devices = ["cpu"]
        elif d == "cpu":
            logger.info("Using CPU for quantization")
    return devices


def _split_linear(args, index: List[TensorInfo], ordered: List[TensorInfo], mtype: Optional[str], logger):
    """AutoAWQ export: (the linear weights of `ordered`, every other tensor of the model, which
    is copied)."""
    if mtype in CONV1D_MODEL_TYPES:
        logger.warning(f"model_type {mtype}: Conv1D projection weights ([in, out]) are copied unquantized")
    linear = {i.name for i in ordered if is_linear_weight(i, args.group_size, mtype)}
    passthrough = [i for i in index if i.name not in linear]
    ordered = [i for i in ordered if i.name in linear]
    logger.info(f"{'GPTQ' if args.output_format == 'gptq' else 'AutoAWQ'} export: {len(ordered)} linear weights "
                f"quantized, {len(passthrough)} copied")
    return ordered, passthrough


def _main_single(args, cfg: StreamSettings, loader, ordered: List[TensorInfo], passthrough: List[TensorInfo],
                 devices: List[str], logger, start: float) -> int:
    """One process: the tensors LPT-partitioned over its devices, one host thread per device."""
    parts = partition_tensors(ordered, len(devices))
    quantizers = {d: new_quantizer(args, d) for d in devices}
    results: Dict[str, Dict[str, torch.Tensor]] = {}
    lock = threading.Lock()
    # chunked output written while later batches are still being read and quantized
    writer = None
    if not cfg.export_autoawq:
        writer = ChunkWriter([i.name for i in ordered], args.output_dir, args.chunk_size, args.save_safetensors,
                             logger, writers=writer_threads(ordered, cfg.packed))
        # the writer owns every result until its chunk is on disk; a device's pipeline may
        # then reuse (wrap) its host output ring — only when it is the writer's only producer
        results = _NullSink()
    threads = []
    TIMINGS["pre_stream_s"] = time.time() - start
    for d, part in zip(devices, parts):
        logger.info(f"Processing {len(part)} tensors on {d}")
        th = threading.Thread(target=_device_worker, args=(cfg, loader, part, quantizers[d], d, results, lock, logger),
                              kwargs={"on_done": writer.done if writer else None,
                                      "writer": writer if len(devices) == 1 else None})
        th.start()
        threads.append(th)
    for th in threads:
        th.join()
    TIMINGS["quantize_s"] = time.time() - start

    quantized = {i.name: results[i.name] for i in ordered if i.name in results}   # size-descending
    if not quantized and writer is not None:
        writer.close()

    def save():
        if writer is None:
            save_autoawq(quantized, loader, passthrough, args.output_dir, args, logger,
                         failed=[i for i in ordered if i.name not in quantized])
            return
        t_close = time.time()
        writer.close()
        if writer.times:
            TIMINGS["writer"] = {"chunks": len(writer.times), "close_wait_s": round(time.time() - t_close, 4),
                                 "write_s_sum": round(sum(e - b for _, b, e in writer.times), 4),
                                 "write_s_max": round(max(e - b for _, b, e in writer.times), 4),
                                 "last_submit_to_end_s": round(max(e for _, _, e in writer.times)
                                                               - max(a for a, _, _ in writer.times), 4)}
            if STREAM_OPTS.get("trace"):   # per chunk: submitted, started, ended (s after `start`)
                TIMINGS["writer"]["trace"] = [tuple(round(v - start, 4) for v in t) for t in writer.times]
    return finish_run(args, ordered, quantized, logger, start, save)


def main(argv: Optional[List[str]] = None) -> int:
    logger = None
    t_main = time.time()
    try:
        args = parse_args(argv)
        logger = get_logger(name="awq_quantizer", level=args.log_level, to_file=args.log_file is not None,
                            file_path=args.log_file)
        os.makedirs(args.output_dir, exist_ok=True)
        err = check_flags(args)     # before any device or model work
        if err:
            logger.error(err)
            return 1

        if args.act_samples and not os.path.isfile(args.act_samples):   # before the model is read
            logger.error(f"--act_samples: {args.act_samples} does not exist")
            return 1

        devices = _pick_devices(args, logger)
        from . import distributed as D
        world = D.env_world()[2]
        if len(devices) == 1 and world <= 1:
            start_warmup(devices[0])    # HIP's first-use costs overlap the index and planning below
        TIMINGS["devices_s"] = round(time.time() - t_main, 4)
        TIMINGS["module_import_torch_s"] = round(_IMPORT_TORCH_S, 4)
        logger.info(f"Loading model from {args.model_id}")
        try:
            loader = load_model_from_hub(args.model_id, logger_level=args.log_level)
            index = loader.tensor_index()
        except Exception as e:  # noqa: BLE001
            logger.error(f"Failed to load model: {e}")
            return 1

        TIMINGS["index_s"] = round(time.time() - t_main - TIMINGS["devices_s"], 4)
        logger.info("Preparing tensors for quantization")
        start = time.time()
        ordered = select_tensors(index, logger)
        autoawq = args.output_format in CHECKPOINT_FORMATS     # a checkpoint export, in either layout
        mtype = model_type_of(loader) if autoawq else None
        err = check_args(args, world, len(devices), mtype)
        passthrough: List[TensorInfo] = []
        if autoawq and err not in (AUTOAWQ_NEEDS_4_BITS, GPTQ_NEEDS_4_BITS):   # that refusal comes before the export is planned and logged
            ordered, passthrough = _split_linear(args, index, ordered, mtype, logger)
        if err:
            logger.error(err)
            return 1

        act_stats = None
        act_samples = None      # --search_loss / --clip_loss output: "<block>.<group>.samples" -> [tokens, in]
        if wants_samples(args):     # loaded (or collected) once, shared by both searches
            act_samples = {}
            if args.act_samples:
                from safetensors.torch import load_file
                act_samples = load_file(args.act_samples)
                logger.info(f"Loaded token samples of {len(act_samples)} inputs from {args.act_samples}")
        if args.calib_ids:
            act_stats = calibrate_for_main(args, devices[0], logger,
                                           samples_out=act_samples if wants_samples(args) else None)
            if act_stats is None:
                return 1
        elif args.act_stats:
            act_stats = load_act_stats(args.act_stats, logger)
        elif args.scale_method == "awq":
            logger.warning("--scale_method awq without --act_stats: every weight is quantized RTN")

        cfg = StreamSettings.from_args(args, packed=args.output_format in ("packed",) + CHECKPOINT_FORMATS,
                                       export_autoawq=autoawq,
                                       export_gptq=args.gptq_format if args.output_format == "gptq" else None, act_stats=act_stats, act_clip=act_clip_of(args))
        if args.fold_scales:
            from .fold_cli import _main_fold_scales
            return _main_fold_scales(args, cfg, loader, index, ordered, passthrough, devices[0], logger, start,
                                     act_samples=act_samples)
        if world > 1:   # torchrun: one process per GPU, LPT shard, RCCL gather to rank 0
            from .dist_cli import _main_distributed
            return _main_distributed(args, cfg, loader, ordered, logger, start, passthrough)
        return _main_single(args, cfg, loader, ordered, passthrough, devices, logger, start)
    except SystemExit:
        raise
    except Exception as e:  # noqa: BLE001
        if logger is None:
            logging.getLogger("awq_quantizer").error(f"Error during quantization: {e}")
        else:
            logger.error(f"Error during quantization: {e}")
        return 1


if __name__ == "__main__":
    sys.exit(main())
