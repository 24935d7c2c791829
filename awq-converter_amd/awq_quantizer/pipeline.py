"""
The per-device quantize loop of the CLI: quantize_stream() runs a list of tensors on one GPU,
on the native pipeline (stream.py, awq_stream_*) or on the Python pipeline below, which drives
the same read -> H2D -> quantize -> D2H stages from Python.  The launch modes (main.py,
fold_cli.py, dist_cli.py) build one StreamSettings per run and call it once per device; results
leave through `out` / `on_done`, and whatever writes them (output.py) is passed in, not imported.
"""

import threading
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import torch

from .model_loading import TensorInfo
from .quantization.awq import AWQQuantizer

TIMINGS: Dict[str, float] = {}   # phase times of the last main() call (scripts/cli_bench.py)
# native pipeline overrides for measurement scripts (scripts/cli_profile.py --stream-opts):
# slot_bytes, nslots, copy_streams (1: H2D and D2H share one stream), trace (1: per-batch
# timestamps, include/awq_hip.h awq_stream_config.trace), readers (pread threads), writers
# (ChunkWriter threads), host_arena (0: one pinned buffer per output chunk)
STREAM_OPTS: Dict[str, int] = {}

OnDone = Optional[Callable[[str, Optional[Dict[str, torch.Tensor]]], None]]


@dataclass(frozen=True)
class StreamSettings:
    """What a run asks of every device's pipeline alike.  act_stats (scale_method="awq"):
    name -> (x_mean, x_sq); those weights take the activation-aware search
    (AWQQuantizer.quantize_layer_group, one weight per layer group) and carry its "input_scale"
    in their results.  act_clip ({"clip_grid", "clip_max_shrink"}): those weights also take the
    activation-aware clip search (quantize_layer_group's clip=True)."""
    readers: int
    lookahead: int
    packed: bool
    memory_efficient: bool = False
    keep_on_device: bool = False
    batch_bytes: int = 1 << 30
    export_autoawq: bool = False         # a checkpoint export: AutoAWQ's GEMM layout, or with export_gptq GPTQ's
    export_gptq: Optional[str] = None    # the GPTQ checkpoint_format ("gptq" / "gptq_v2")
    act_stats: Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor]]] = None
    act_clip: Optional[Dict[str, float]] = None
    engine: str = "native"

    @classmethod
    def from_args(cls, args, **fields) -> "StreamSettings":
        """The CLI's flags; `fields` are what the launch mode decides."""
        return cls(readers=args.num_workers, lookahead=max(1, args.prefetch_factor * args.batch_size),
                   memory_efficient=args.memory_efficient, engine=args.stream_engine, **fields)


def new_quantizer(args, device: str) -> AWQQuantizer:
    """The CLI's AWQQuantizer for one device."""
    return AWQQuantizer(bits=args.bits, group_size=args.group_size, symmetric=args.symmetric,
                        zero_point=args.zero_point, percentile=args.percentile, scale_method=args.scale_method,
                        per_channel=args.per_channel, device=device, search_grid=args.search_grid,
                        search_max_shrink=args.search_max_shrink, duo_scaling=not args.no_duo_scaling,
                        logger_name=f"awq_quantizer_{device}", logger_level=args.log_level,
                        logger_to_file=args.log_file is not None, logger_file_path=args.log_file)


def _batches(infos: List[TensorInfo], budget: int) -> List[List[TensorInfo]]:
    """Consecutive runs of tensors (processing order kept) of at most `budget` input bytes
    (a larger tensor forms a batch of its own)."""
    out, cur, size = [], [], 0
    for info in infos:
        if cur and size + info.nbytes > budget:
            out.append(cur)
            cur, size = [], 0
        cur.append(info)
        size += info.nbytes
    if cur:
        out.append(cur)
    return out


def _batch_budget(total: int, batch_bytes: int) -> int:
    """Input bytes per batch: small enough that a small model still pipelines (read / H2D /
    kernel / D2H of neighbouring batches overlap) — about 8 batches per device, 32 MiB ..
    batch_bytes each."""
    return max(32 << 20, min(batch_bytes, total // 8))


def _pinned_copy(t: torch.Tensor) -> torch.Tensor:
    """Host copy in page-locked memory (torch's caching host allocator), so the H2D / D2H
    copies run asynchronously on the copy stream."""
    p = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    p.copy_(t)
    return p


def _with_input_scale(exported: Dict[str, torch.Tensor], packed: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    if "input_scale" in packed:
        exported["input_scale"] = packed["input_scale"]
    return exported


def quantize_stream_native(loader, infos: List[TensorInfo], quantizer: AWQQuantizer, device: str, readers: int,
                           packed: bool, out: Dict, lock: threading.Lock, logger, keep_on_device: bool = False,
                           on_done: OnDone = None, writer=None, slot_bytes: int = 0, host_ring_bytes: int = 0,
                           dev_ring_bytes: int = 0) -> None:
    """The CLI's read -> quantize -> collect loop on the native pipeline with bounded output
    memory (awq_quantizer/stream.py).  With `writer` (the ChunkWriter that consumes
    `on_done`'s results) the host ring may wrap: results are released once their chunk is
    written; without it the host ring holds the whole output."""
    from .stream import quantize_stream_native as run
    hook = groups = None
    if writer is not None and not keep_on_device:
        hook = writer.add_written_hook
        groups = writer.predict_groups
    run(loader, infos, quantizer, device, readers, packed, out, lock, logger, keep_on_device=keep_on_device,
        on_done=on_done, release_hook=hook, group_of=groups, slot_bytes=slot_bytes,
        host_ring_bytes=host_ring_bytes or int(STREAM_OPTS.get("host_ring_bytes", 0)),
        dev_ring_bytes=dev_ring_bytes or int(STREAM_OPTS.get("dev_ring_bytes", 0)),
        opts=STREAM_OPTS, timings=TIMINGS)


def quantize_stream(cfg: StreamSettings, loader, infos: List[TensorInfo], quantizer: AWQQuantizer, device: str,
                    out: Dict, lock: threading.Lock, logger, on_done: OnDone = None, writer=None) -> None:
    """Quantize `infos` on one GPU.  RTN and the per-group clip search (scale_method
    "search") to the packed or reference format run on the native pipeline
    (quantize_stream_native; `writer`: the ChunkWriter consuming on_done, whose written
    chunks release the pipeline's host ring — only when it serves this device alone); the
    activation-aware search (`act_stats`), the AutoAWQ export and `engine="python"` on the
    Python pipeline below."""
    if cfg.engine == "native" and not cfg.act_stats and not cfg.export_autoawq and hasattr(loader, "data_location"):
        return quantize_stream_native(loader, infos, quantizer, device, cfg.readers, cfg.packed, out, lock, logger,
                                      keep_on_device=cfg.keep_on_device, on_done=on_done, writer=writer)
    return quantize_stream_python(cfg, loader, infos, quantizer, device, out, lock, logger, on_done)


def _device_worker(cfg: StreamSettings, loader, infos: List[TensorInfo], quantizer: AWQQuantizer, device: str,
                   out: Dict, lock: threading.Lock, logger, on_done: OnDone = None, writer=None) -> None:
    """Thread body of one device: a failure of the whole device (no GPU, no library) is
    logged; its tensors then count as not quantized."""
    try:
        quantize_stream(cfg, loader, infos, quantizer, device, out, lock, logger, on_done=on_done, writer=writer)
    except Exception as e:  # noqa: BLE001
        if logger:
            logger.error(f"Quantization on {device} failed: {e}")


# ---- the Python pipeline: the steps of one batch, in the order quantize_stream_python runs them ----

def _view(buf: torch.Tensor, off: int, info: TensorInfo) -> torch.Tensor:
    return buf[off:off + info.nbytes].view(info.dtype).view(info.shape)


def _submit_reads(pool: ThreadPoolExecutor, loader, batch: List[TensorInfo]):
    """Plan and stage a batch (host, no stream): every tensor's read goes to the reader pool.  A
    loader with direct reads fills slices of one pinned staging buffer, so the batch is one H2D;
    any other loader's read is followed by a pinned copy.  Returns ([(info, future)], staging),
    staging = (pinned uint8 buffer, name -> byte offset) or None."""
    if not hasattr(loader, "read_pinned"):
        return [(info, pool.submit(lambda i: _pinned_copy(loader.read(i)), info)) for info in batch], None
    offs, pos = {}, 0
    for info in batch:
        if info.dtype is None:
            continue
        offs[info.name] = pos
        pos += (info.nbytes + 255) // 256 * 256      # 256-B aligned slices (16-B vector loads)
    buf = torch.empty(max(pos, 1), dtype=torch.uint8, pin_memory=True)
    # straight from the file into pinned memory (one copy): into the staging buffer where the
    # tensor has a slice of it
    reads = [(info, pool.submit(loader.read_into, info, _view(buf, offs[info.name], info)) if info.name in offs
              else pool.submit(loader.read_pinned, info)) for info in batch]
    return reads, (buf, offs)


def _collect_reads(reads, device: str, logger, on_done: OnDone) -> Dict[str, torch.Tensor]:
    """Wait for a batch's reads (host, no stream): name -> pinned host tensor; a tensor whose
    read failed is logged, reported to on_done as failed and left out."""
    host = {}
    for info, fut in reads:
        try:
            host[info.name] = fut.result()
        except Exception as e:  # noqa: BLE001
            if logger:
                logger.error(f"Failed to quantize tensor {info.name} on {device}: {e}")
            if on_done:
                on_done(info.name, None)
    return host


def _upload(host: Dict[str, torch.Tensor], batch: List[TensorInfo], staging, dev: torch.device,
            copy_stream: "torch.cuda.Stream"):
    """H2D on the copy stream, then ev_in recorded there.  Returns (name -> device tensor, the
    pinned staging buffer to keep alive until the copy is done or None, ev_in)."""
    staged = None
    with torch.cuda.stream(copy_stream):
        if staging is not None:     # the whole staging buffer in one copy; device views of it
            buf, offs = staging
            dbuf = torch.empty(buf.numel(), dtype=torch.uint8, device=dev)
            dbuf.copy_(buf, non_blocking=True)
            by_name = {i.name: i for i in batch}
            dev_in = {n: _view(dbuf, offs[n], by_name[n]) for n in host}
            staged = buf
        else:
            dev_in = {n: t.to(dev, non_blocking=True) for n, t in host.items()}
        ev_in = torch.cuda.Event()
        ev_in.record(copy_stream)
    return dev_in, staged, ev_in


def _quantize(cfg: StreamSettings, quantizer: AWQQuantizer, dev_in: Dict[str, torch.Tensor],
              compute: "torch.cuda.Stream", ev_in: "torch.cuda.Event", logger):
    """The compute stream waits for ev_in, runs the batch's kernels (the activation-aware search
    weight by weight, one ragged launch per dtype for the rest, then the AutoAWQ export) and
    records ev_k.  Returns (name -> device result dict, ev_k); a weight whose search raised is
    logged and missing from the results."""
    act_stats = cfg.act_stats
    clip_kw = {"clip": True, "clip_grid": int(cfg.act_clip["clip_grid"]),
               "clip_max_shrink": float(cfg.act_clip["clip_max_shrink"])} if cfg.act_clip else {}
    compute.wait_event(ev_in)
    with torch.cuda.stream(compute):
        searched = {}
        for name in [n for n in dev_in if act_stats and n in act_stats]:
            try:
                xm, xs = act_stats[name]
                searched[name] = quantizer.quantize_layer_group(
                    {name: dev_in[name]}, x_mean=xm, x_sq=xs, packed=cfg.packed, **clip_kw)["results"][name]
            except Exception as e:  # noqa: BLE001  (reference semantics: skip and continue)
                if logger:
                    logger.error(f"Error quantizing tensor: {name}, error: {e}")
        res = quantizer.quantize_model_device({n: t for n, t in dev_in.items()
                                               if not (act_stats and n in act_stats)}, packed=cfg.packed)
        res.update(searched)
        if cfg.export_gptq:
            res = {n: _with_input_scale(quantizer.export_gptq(r, cfg.export_gptq), r) for n, r in res.items()}
        elif cfg.export_autoawq:
            res = {n: _with_input_scale(quantizer.export_autoawq(r), r) for n, r in res.items()}
        ev_k = torch.cuda.Event()
        ev_k.record(compute)
    return res, ev_k


def _download(res: Dict[str, Dict[str, torch.Tensor]], copy_stream: "torch.cuda.Stream", ev_k: "torch.cuda.Event"):
    """The copy stream waits for ev_k, copies every device tensor of the results into pinned host
    memory (D2H) and records ev_out.  Returns (name -> host result dict, ev_out); the host
    tensors hold their values once ev_out has completed."""
    copy_stream.wait_event(ev_k)
    with torch.cuda.stream(copy_stream):
        host_res = {}
        for name, r in res.items():
            hr = {}
            for f, v in r.items():
                if isinstance(v, torch.Tensor) and v.is_cuda:
                    h = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
                    h.copy_(v, non_blocking=True)
                    hr[f] = h
                else:
                    hr[f] = v
            host_res[name] = hr
        ev_out = torch.cuda.Event()
        ev_out.record(copy_stream)
    return host_res, ev_out


def _finish(entry, out: Dict, lock: threading.Lock, device: str, logger, on_done: OnDone) -> float:
    """Host: wait for a batch's ev_out, then publish its results (out, the log line and on_done
    per tensor).  Returns the seconds waited.  Dropping `entry` afterwards releases the batch's
    inputs and device results, which it kept alive until their copies were done."""
    results, ev_out, _keep = entry
    t0 = time.perf_counter()
    ev_out.synchronize()
    waited = time.perf_counter() - t0
    with lock:
        out.update(results)
    for name in results:
        if logger:
            logger.info(f"Successfully quantized tensor: {name} on {device}")
        if on_done:
            on_done(name, results[name])
    return waited


def quantize_stream_python(cfg: StreamSettings, loader, infos: List[TensorInfo], quantizer: AWQQuantizer,
                           device: str, out: Dict, lock: threading.Lock, logger, on_done: OnDone = None) -> None:
    """Quantize `infos` on one GPU as a pipeline over batches of tensors (<= batch_bytes of
    input each):

      reader threads: safetensors read -> pinned host copy      (batch k+1 .. k+lookahead)
      copy stream:    H2D of batch k                            (overlaps batch k-1's kernels)
      compute stream: one ragged launch per dtype for batch k   (awq_quantize_ragged)
      copy stream:    D2H of batch k's results into pinned host memory

    The reference instead loads every file whole and copies every tensor to the device
    eagerly (main.py:296-307), then quantizes tensor by tensor.  Per-tensor failures are
    logged and skipped (main.py:387-390).  One batch's D2H stays in flight while the next is
    submitted; its results are published (_finish) after that."""
    t_enter = time.perf_counter()
    if not (device.startswith("cuda") and torch.cuda.is_available()):
        quantizer.compute_device()   # raises HipUnavailable: no CPU path
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    torch.cuda.set_device(dev)
    copy_stream = torch.cuda.Stream(dev)
    compute = torch.cuda.current_stream(dev)
    budget = _batch_budget(sum(i.nbytes for i in infos), cfg.batch_bytes)
    batches = _batches(infos, budget)
    depth = max(1, cfg.lookahead // max(1, max(len(b) for b in batches) if batches else 1))
    clock = time.perf_counter
    t_read = t_submit = t_finish = 0.0
    inflight = deque()

    with ThreadPoolExecutor(max_workers=max(1, cfg.readers)) as pool:
        pending = {}   # batch -> its reads and staging buffer

        def submit(k):
            if k < len(batches) and k not in pending:
                pending[k] = _submit_reads(pool, loader, batches[k])

        for k in range(min(len(batches), depth + 1)):
            submit(k)
        for k in range(len(batches)):
            submit(k + depth)
            reads, staging = pending.pop(k)
            t0 = clock()
            host = _collect_reads(reads, device, logger, on_done)
            t1 = clock()
            t_read += t1 - t0
            if not host:
                continue
            if logger:
                for name in host:
                    logger.info(f"Quantizing tensor: {name} on {device}")
            dev_in, staged, ev_in = _upload(host, batches[k], staging, dev, copy_stream)
            res, ev_k = _quantize(cfg, quantizer, dev_in, compute, ev_in, logger)
            for name in host:
                if name not in res:
                    if logger:
                        logger.error(f"Failed to quantize tensor {name} on {device}")
                    if on_done:
                        on_done(name, None)
            if cfg.keep_on_device:
                ev_k.synchronize()
                with lock:
                    out.update(res)
                continue
            host_res, ev_out = _download(res, copy_stream, ev_k)
            t_submit += clock() - t1
            # inputs and device results stay referenced until their copies are done
            inflight.append((host_res, ev_out, (host, dev_in, res, staged)))
            while len(inflight) > 1:
                t_finish += _finish(inflight.popleft(), out, lock, device, logger, on_done)
            if cfg.memory_efficient:
                torch.cuda.empty_cache()
        while inflight:
            t_finish += _finish(inflight.popleft(), out, lock, device, logger, on_done)
    # host-side phase times of this device's pipeline (scripts/cli_bench.py prints them)
    TIMINGS.update({f"stream_{device}": {"wall_s": round(time.perf_counter() - t_enter, 4),
                                          "batches": len(batches), "batch_MB": budget >> 20,
                                          "read_wait_s": round(t_read, 4), "submit_s": round(t_submit, 4),
                                          "finish_wait_s": round(t_finish, 4)}})
