"""
Everything the CLI writes: chunk files + metadata.json (the reference layout, main.py:430-512),
safetensors chunks, the streaming ChunkWriter, and AutoAWQ checkpoints.  The launch modes
(main.py, fold_cli.py, dist_cli.py) call these; the per-device pipeline (pipeline.py) is handed
a writer and never imports this module.
"""

import json
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import ptfile
from .model_loading import TensorInfo
from .pipeline import STREAM_OPTS, TIMINGS


def _flatten(tensors: Dict[str, Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
    flat = {}
    for name, d in tensors.items():
        for k, v in d.items():
            flat[f"{name}.{k}"] = v.contiguous()
    return flat


def save_model_in_chunks(tensors: Dict[str, Dict[str, torch.Tensor]], output_dir: str, chunk_size: int = 10,
                         use_safetensors: bool = False, logger=None) -> None:
    """model_chunk_NNNN.{pt|safetensors} + metadata.json (reference main.py:430-512)."""
    os.makedirs(output_dir, exist_ok=True)
    names = list(tensors)
    num_chunks = (len(names) + chunk_size - 1) // chunk_size
    if logger:
        logger.info(f"Saving model in {num_chunks} chunks with {chunk_size} tensors per chunk")
    first = next(iter(tensors.values()))
    qparams = {k: (first[k].item() if k in first else None) for k in ("bits", "group_size", "symmetric")}
    tensor_to_chunk = {}
    # chunk files are independent: written by a small thread pool (ptfile.save: the archive is
    # written by native code that releases the GIL)
    with ThreadPoolExecutor(max_workers=min(8, max(2, cpu_share() // 2))) as pool:
        futs = []
        for c in range(num_chunks):
            chunk_names = names[c * chunk_size:(c + 1) * chunk_size]
            for n in chunk_names:
                tensor_to_chunk[n] = c
            futs.append(pool.submit(_write_chunk, {n: tensors[n] for n in chunk_names}, output_dir, c,
                                    use_safetensors, logger, f"{c + 1}/{num_chunks}"))
        for f in futs:
            f.result()
    _write_metadata(output_dir, num_chunks, chunk_size, tensor_to_chunk, use_safetensors, len(names), qparams,
                    logger)


CHUNK_STEM = "model_chunk_{:04d}"   # reference main.py:485


def _chunk_path(output_dir: str, c: int, use_safetensors: bool, stem: str = CHUNK_STEM) -> str:
    return os.path.join(output_dir, stem.format(c) + (".safetensors" if use_safetensors else ".pt"))


_ST_DTYPE = {torch.int32: "I32", torch.int64: "I64", torch.int16: "I16", torch.int8: "I8", torch.uint8: "U8",
             torch.bool: "BOOL", torch.float16: "F16", torch.bfloat16: "BF16", torch.float32: "F32",
             torch.float64: "F64"}


def save_safetensors(flat: Dict[str, torch.Tensor], path: str) -> None:
    """A safetensors file (8-byte header length, JSON header, the tensors' bytes back to back)
    written straight from the tensors' memory: tensors may be views of one buffer (the native
    pipeline's chunk buffers), which safetensors.torch.save_file refuses to write."""
    import numpy as np
    header, off, parts = {}, 0, []
    for name in sorted(flat):
        t = flat[name].detach().cpu().contiguous()
        nb = t.numel() * t.element_size()
        header[name] = {"dtype": _ST_DTYPE[t.dtype], "shape": list(t.shape), "data_offsets": [off, off + nb]}
        parts.append(t)
        off += nb
    header["__metadata__"] = {"format": "pt"}
    h = json.dumps(header, separators=(",", ":")).encode()
    h += b" " * (-len(h) % 8)
    with open(path, "wb") as f:
        f.write(len(h).to_bytes(8, "little"))
        f.write(h)
        for t in parts:
            if t.numel():
                raw = t.reshape(-1).view(torch.uint8) if t.dtype != torch.bool else t.reshape(-1).to(torch.uint8)
                f.write(memoryview(np.ascontiguousarray(raw.numpy())))


def _write_chunk(chunk: Dict[str, Dict[str, torch.Tensor]], output_dir: str, c: int, use_safetensors: bool,
                 logger=None, label: str = "", stem: str = CHUNK_STEM) -> None:
    path = os.path.join(output_dir, stem.format(c))
    if use_safetensors:
        save_safetensors(_flatten(chunk), path + ".safetensors")
        if logger:
            logger.info(f"Saved chunk {label or c + 1} with {len(chunk)} tensors in safetensors format")
    else:
        ptfile.save(chunk, path + ".pt")        # torch.save's archive, written without the GIL
        if logger:
            logger.info(f"Saved chunk {label or c + 1} with {len(chunk)} tensors in PyTorch format")


def _write_metadata(output_dir, num_chunks, chunk_size, tensor_to_chunk, use_safetensors, num_tensors, qparams,
                    logger=None) -> None:
    meta = {"num_chunks": num_chunks, "chunk_size": chunk_size, "tensor_to_chunk": tensor_to_chunk,
            "format": "safetensors" if use_safetensors else "pytorch", "num_tensors": num_tensors,
            "quantization_params": qparams}
    with open(os.path.join(output_dir, "metadata.json"), "w") as f:
        json.dump(meta, f, indent=2)
    if logger:
        logger.info("Saved metadata file with tensor mapping")


class ChunkWriter:
    """save_model_in_chunks while the GPU pipeline is still running: a writer thread walks the
    tensors in processing order (bytes descending, main.py:259) and writes chunk c as soon as
    its chunk_size successful tensors are on the host, so disk writes overlap the reads and
    kernels of later batches.  Output files and metadata.json are identical to
    save_model_in_chunks on the finished dict (failed tensors are skipped in the same order;
    chunk numbers are only known once every earlier tensor has finished).  Complete chunks
    are written by a small thread pool: ptfile.save builds the pickle stream in Python and
    writes the archive natively without the GIL, so chunks serialise in parallel (5.4 MB
    packed chunks in the build container: torch.save 0.72 / 1.2 GB/s on 1 / 8 threads,
    ptfile 1.5 / 5.1 GB/s).

    stem / metadata: torchrun's per-rank mode writes under a rank-private file stem and no
    metadata.json; after close(), `t2c` (name -> local chunk), `n_chunks`, `n_ok` and
    `qparams` describe what was written (dist_cli._commit_rank_chunks renumbers the files)."""

    def __init__(self, order: List[str], output_dir: str, chunk_size: int, use_safetensors: bool, logger=None,
                 writers: int = 0, stem: str = CHUNK_STEM, metadata: bool = True):
        self.order, self.dir, self.size, self.st, self.logger = order, output_dir, chunk_size, use_safetensors, logger
        self.writers = writers or min(8, max(2, cpu_share() // 2))
        # while producers run, at most `writers` chunk writes at once (more stalled the GPU
        # pipeline's HIP calls); once close() is called the backlog drains with tail_writers
        self.tail_writers = max(self.writers, min(8, max(2, cpu_share() // 2)))
        self.gate = threading.Semaphore(self.writers)
        self.stem, self.metadata = stem, metadata
        self.t2c: Dict[str, int] = {}
        self.n_chunks = self.n_ok = 0
        self.qparams: Optional[Dict] = None
        self.status: Dict[str, Optional[Dict[str, torch.Tensor]]] = {}
        self.closed = False
        self.error: Optional[BaseException] = None
        self.cv = threading.Condition()
        self.times: List[Tuple[float, float, float]] = []   # per chunk: submitted, started, ended (time.time)
        self.failed: set = set()
        self.hooks: List[Callable[[List[str]], None]] = []
        self.n_reported = 0
        self.widened = False
        os.makedirs(output_dir, exist_ok=True)
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def done(self, name: str, result: Optional[Dict[str, torch.Tensor]]) -> None:
        """A tensor finished: its host result dict, or None if it failed.  Once every tensor
        has reported, the producers' HIP work is over: the pool widens for the tail.  Raises
        once a chunk write has failed, so the producer stops (the native pipeline then cancels
        its remaining batches) instead of quantizing into a run that cannot be saved."""
        with self.cv:
            if self.error is not None:
                raise RuntimeError(f"chunk writer failed: {self.error}") from self.error
            self.status[name] = result
            if result is None:
                self.failed.add(name)
            self.n_reported += 1
            last = self.n_reported == len(self.order)
            self.cv.notify()
        if last:
            self._widen()

    def _widen(self) -> None:
        with self.cv:
            if self.widened:
                return
            self.widened = True
        for _ in range(self.tail_writers - self.writers):
            self.gate.release()

    def add_written_hook(self, fn: Callable[[List[str]], None]) -> None:
        """fn(names) after each chunk file is written: its results are no longer read."""
        with self.cv:
            self.hooks.append(fn)

    def predict_groups(self) -> Dict[str, int]:
        """The chunk every tensor not yet known to have failed lands in, if it succeeds."""
        with self.cv:
            failed = set(self.failed)
        out, k = {}, 0
        for name in self.order:
            if name not in failed:
                out[name] = k // self.size
                k += 1
        return out

    def _run(self) -> None:
        try:
            with ThreadPoolExecutor(max_workers=self.tail_writers) as pool:
                futs = []
                chunk, c, t2c, qparams, n_ok = {}, 0, {}, None, 0
                for name in self.order:
                    with self.cv:
                        while name not in self.status and not self.closed:
                            self.cv.wait()
                        res = self.status.pop(name, None)
                    if res is None:
                        continue
                    if qparams is None:
                        qparams = {k: (res[k].item() if k in res else None) for k in ("bits", "group_size", "symmetric")}
                    chunk[name] = res
                    t2c[name] = c
                    n_ok += 1
                    if len(chunk) == self.size:
                        futs.append(pool.submit(self._timed_write, chunk, c, time.time()))
                        chunk, c = {}, c + 1
                if chunk:
                    futs.append(pool.submit(self._timed_write, chunk, c, time.time()))
                    c += 1
                for f in futs:
                    f.result()
            self.t2c, self.n_chunks, self.n_ok, self.qparams = t2c, c, n_ok, qparams
            if n_ok and self.metadata:
                _write_metadata(self.dir, c, self.size, t2c, self.st, n_ok, qparams, self.logger)
        except BaseException as e:  # noqa: BLE001  (reported by close())
            with self.cv:
                if self.error is None:
                    self.error = e
            # nothing more will be written: release every result, so a producer blocked on a
            # wrapping host ring (awq_stream_release) is never left waiting for this thread
            self._report_written(list(self.order))

    def _report_written(self, names: List[str]) -> None:
        with self.cv:
            hooks = list(self.hooks)
        for fn in hooks:
            fn(names)

    def _timed_write(self, chunk, c: int, t_submit: float) -> None:
        names = list(chunk)
        try:
            with self.gate:
                t0 = time.time()
                _write_chunk(chunk, self.dir, c, self.st, self.logger, stem=self.stem)
                self.times.append((t_submit, t0, time.time()))
        except BaseException as e:  # noqa: BLE001  (first error wins; done() and close() report it)
            with self.cv:
                if self.error is None:
                    self.error = e
            raise
        finally:
            # written or failed, these results are never read again: the pipeline may reuse
            # their ring range (a failed write must not leave it blocked)
            chunk.clear()
            self._report_written(names)

    def close(self) -> None:
        """Every producer has finished: unfinished tensors count as failed; wait for the writes."""
        with self.cv:
            self.closed = True
            self.cv.notify()
        self._widen()                                       # the producers are done: widen the pool
        self.thread.join()
        if self.error is not None:
            raise self.error


class _NullSink(dict):
    """quantize_stream's result dict when a ChunkWriter already owns every result: it keeps
    the names only (the results may be views of a ring the pipeline reuses once written)."""

    def __setitem__(self, name, value) -> None:
        super().__setitem__(name, None)

    def update(self, *a, **k) -> None:
        for d in a + (k,):
            for name in d:
                super().__setitem__(name, None)


def _rank_stem(rank: int) -> str:
    """Rank-private chunk file stem (renamed to CHUNK_STEM numbers once all ranks agree)."""
    return f".rank{rank:05d}_chunk_{{:04d}}"


def _to_cpu(d: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def model_type_of(loader) -> Optional[str]:
    """config.json's model_type next to the weights, if any."""
    path = os.path.join(getattr(loader, "model_path", "") or "", "config.json")
    try:
        with open(path) as f:
            return json.load(f).get("model_type")
    except (OSError, ValueError):
        return None


def autoawq_tensors(quantized: Dict[str, Dict[str, torch.Tensor]], loader, passthrough: List[TensorInfo],
                    failed: List[TensorInfo] = (),
                    overrides: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """The tensors of an AutoAWQ checkpoint (or one shard of it): `<layer>.qweight/.qzeros/
    .scales` per quantized linear weight; every passthrough tensor and every linear weight
    that failed to quantize copied unchanged (those layers stay unquantized:
    modules_to_not_convert).  overrides (--fold_scales): name -> tensor written in place of
    the source's (norm weights and biases with 1 / s folded in)."""
    tensors = {}
    for name, r in quantized.items():
        prefix = name[: -len(".weight")]
        for f in ("qweight", "qzeros", "scales") + (("g_idx",) if "g_idx" in r else ()):   # g_idx: the GPTQ layout
            tensors[f"{prefix}.{f}"] = r[f].contiguous()
    for info in list(passthrough) + list(failed):
        if overrides and info.name in overrides:
            tensors[info.name] = overrides[info.name].contiguous()
        else:
            tensors[info.name] = loader.read(info).contiguous()
    return tensors


def write_autoawq_configs(output_dir: str, args, loader, not_converted: List[str], logger=None) -> None:
    """quant_config.json (AutoAWQ) and, when the source has one, config.json with a
    transformers `quantization_config`; `not_converted` = module names of linear weights
    left unquantized (their quantization failed and they were copied through)."""
    qcfg = {"zero_point": not args.symmetric, "q_group_size": args.group_size, "w_bit": 4, "version": "GEMM"}
    if not_converted:
        qcfg["modules_to_not_convert"] = list(not_converted)
    with open(os.path.join(output_dir, "quant_config.json"), "w") as f:
        json.dump(qcfg, f, indent=2)
    src = os.path.join(getattr(loader, "model_path", "") or "", "config.json")
    if os.path.isfile(src):
        with open(src) as f:
            cfg = json.load(f)
        cfg["quantization_config"] = {"quant_method": "awq", "bits": 4, "group_size": args.group_size,
                                      "zero_point": not args.symmetric, "version": "gemm"}
        if not_converted:
            cfg["quantization_config"]["modules_to_not_convert"] = list(not_converted)
        with open(os.path.join(output_dir, "config.json"), "w") as f:
            json.dump(cfg, f, indent=2)
    if not_converted and logger:
        logger.warning(f"{len(not_converted)} linear weight(s) failed to quantize and were copied unquantized "
                       f"(modules_to_not_convert): {not_converted}")


def write_gptq_configs(output_dir: str, args, loader, not_converted: List[str], zeros_at_0: Dict[str, int],
                       logger=None) -> None:
    """quantize_config.json (AutoGPTQ) and, when the source has one, config.json with a transformers
    `quantization_config`.  zeros_at_0: layer -> zero points equal to 0, which checkpoint_format
    "gptq" stores as 15 (loaders differ on masking after they add 1): warned about per tensor and
    recorded under "zero_points_at_0"."""
    qcfg = {"quant_method": "gptq", "bits": 4, "group_size": args.group_size, "sym": bool(args.symmetric),
            "desc_act": False, "checkpoint_format": args.gptq_format}
    if not_converted:
        qcfg["modules_to_not_convert"] = list(not_converted)
    zeros_at_0 = {k: int(v) for k, v in zeros_at_0.items() if int(v)}
    meta = {"zero_points_at_0": sum(zeros_at_0.values()), "zero_points_at_0_per_tensor": zeros_at_0}
    with open(os.path.join(output_dir, "quantize_config.json"), "w") as f:
        json.dump(dict(qcfg, meta=meta), f, indent=2)
    src = os.path.join(getattr(loader, "model_path", "") or "", "config.json")
    if os.path.isfile(src):
        with open(src) as f:
            cfg = json.load(f)
        cfg["quantization_config"] = dict(qcfg)
        with open(os.path.join(output_dir, "config.json"), "w") as f:
            json.dump(cfg, f, indent=2)
    if logger:
        for layer, n in zeros_at_0.items():
            logger.warning(f"{layer}: {n} zero point(s) equal to 0 are stored as 15 (checkpoint_format gptq "
                           f"stores zero - 1); a loader must mask to 4 bits after adding 1")
        if not_converted:
            logger.warning(f"{len(not_converted)} linear weight(s) failed to quantize and were copied unquantized "
                           f"(modules_to_not_convert): {not_converted}")


def save_autoawq(quantized: Dict[str, Dict[str, torch.Tensor]], loader, passthrough: List[TensorInfo],
                 output_dir: str, args, logger=None, failed: List[TensorInfo] = (),
                 overrides: Optional[Dict[str, torch.Tensor]] = None) -> None:
    """model.safetensors with `<layer>.qweight/.qzeros/.scales` for every quantized linear
    weight and every other tensor copied unchanged (linear weights that failed to quantize
    included, listed in modules_to_not_convert so the checkpoint still loads), plus the
    configs of write_autoawq_configs.  --output_format gptq: the results are export_gptq()'s
    (`.g_idx` too) and the configs write_gptq_configs'."""
    from safetensors.torch import save_file
    gptq = getattr(args, "output_format", None) == "gptq"
    tensors = autoawq_tensors(quantized, loader, passthrough, failed, overrides)
    save_file(tensors, os.path.join(output_dir, "model.safetensors"), metadata={"format": "pt"})
    not_converted = [i.name[: -len(".weight")] for i in failed]
    if gptq:
        write_gptq_configs(output_dir, args, loader, not_converted,
                           {n[: -len(".weight")]: int(r.get("zero_points_at_0", 0)) for n, r in quantized.items()},
                           logger)
    else:
        write_autoawq_configs(output_dir, args, loader, not_converted, logger)
    if logger:
        logger.info(f"Saved {'GPTQ' if gptq else 'AutoAWQ'} checkpoint: {len(quantized)} quantized linear weights, "
                    f"{len(passthrough) + len(failed)} tensors copied")


def cpu_share() -> int:
    """CPUs this process may actually use: its affinity set, capped by a cgroup v2 CPU quota
    (`cpu.max`) — os.cpu_count() reports the whole machine, which on a shared GPU node is
    many times the process's share."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def writer_threads(infos: List[TensorInfo], packed: bool) -> int:
    """Chunk-writer threads for an output of this size: more writers only pay when the
    files are large — below ~2 GB of output, 8 concurrent writers stalled the pipeline's
    HIP calls for 8-12 ms at a time while 3-4 did not (opt-350m, profiles/round3/r3o: 0.057 s
    vs 0.066-0.072 s warm), and above it the writes are the bound (Llama-3-8B packed 0.36 s
    at 8 writers vs 0.42-0.46 at 4).  STREAM_OPTS["writers"] overrides."""
    forced = STREAM_OPTS.get("writers")
    if forced:
        return int(forced)
    in_bytes = sum(i.nbytes for i in infos)
    out_bytes = in_bytes * (0.26 if packed else 2.05)   # 4-bit packed ~ in / 4; reference ~ 2 x in
    share = cpu_share()
    return min(4, max(2, share // 4)) if out_bytes < (2 << 30) else min(8, max(2, share // 2))


def run_metrics(ordered, quantized, timings) -> Dict[str, float]:
    """One JSON line per run (SURVEY.md §5 metrics): tensors quantized, their input bytes, the
    quantize phase (read + H2D + kernels + D2H, overlapped) and the whole run incl. the final
    writes, and the end-to-end rate over the input bytes.  (Not the kernel's roofline: that is
    bench.py's, with inputs resident in HBM.)"""
    nbytes = sum(i.nbytes for i in ordered if i.name in quantized)
    total = max(float(timings.get("total_s", 0.0)), 1e-9)
    return {"tensors": len(quantized), "input_bytes": int(nbytes),
            "quantize_s": round(float(timings.get("quantize_s", 0.0)), 4), "total_s": round(total, 4),
            "input_GB_per_s": round(nbytes / total / 1e9, 3)}


def finish_run(args, ordered: List[TensorInfo], quantized, logger, start: float,
               save: Optional[Callable[[], None]] = None, **extra_metrics) -> int:
    """How every launch mode ends, and its exit code: nothing quantized is an error; `save()`
    writes the checkpoint (a failure is logged and is the other error); then the run's time and
    its metrics line.  torchrun's rank 0 has saved already when it gets here (save=None) and
    adds `world` to the metrics."""
    if not quantized:
        logger.error("No tensors were successfully quantized")
        return 1
    if save is not None:
        logger.info(f"Successfully quantized {len(quantized)} tensors")
        logger.info(f"Saving quantized model to {args.output_dir}")
        try:
            save()
        except Exception as e:  # noqa: BLE001
            logger.error(f"Failed to save quantized model: {e}")
            return 1
    TIMINGS["total_s"] = time.time() - start
    logger.info(f"Quantization complete in {time.time() - start:.2f} seconds")
    logger.info("metrics " + json.dumps(dict(run_metrics(ordered, quantized, TIMINGS), **extra_metrics)))
    return 0
