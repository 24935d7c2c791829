"""
The CLI under torchrun: one process per GPU, each quantizing its shard, and the three ways the
ranks commit one checkpoint (per-rank chunk files, per-rank AutoAWQ shards, gather to rank 0).
main() imports this module only when WORLD_SIZE > 1; the collectives are distributed.py's.
"""

import json
import os
import threading
import time
from dataclasses import replace
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from . import distributed as D
from . import pipeline
from .model_loading import TensorInfo
from .output import (ChunkWriter, _chunk_path, _NullSink, _rank_stem, _to_cpu, _write_metadata, autoawq_tensors,
                     finish_run, save_autoawq, save_model_in_chunks, write_autoawq_configs, writer_threads)
from .pipeline import TIMINGS, StreamSettings, new_quantizer

_SCALARS = ("bits", "group_size", "symmetric", "shape")


def _main_distributed(args, cfg: StreamSettings, loader, ordered: List[TensorInfo], logger, start: float,
                      passthrough: Optional[List[TensorInfo]] = None) -> int:
    """torchrun mode: one process per GPU; rank r quantizes the tensors an LPT partition by
    bytes assigns it (identical on every rank, derived from the header index with no
    exchange; the reference's own partition_tensors, main.py:395-427).  Output
    (--dist_output):

      per_rank (default): every rank writes its own results as they come off its GPU
        (ChunkWriter under a rank-private file stem, disk writes overlapping its later
        batches); one all_gather_object of the per-rank chunk tables, then each rank renames
        its files to global chunk numbers (rank r's chunks follow rank r-1's) and rank 0
        writes metadata.json over every tensor in processing order (reference main.py:
        430-512).  No result bytes cross the fabric.  AutoAWQ: one safetensors shard per rank
        + model.safetensors.index.json.
      gather: every result is sent to rank 0 in one batched point-to-point round over RCCL
        (xGMI) and rank 0 writes the single-process layout.

    A rank whose pipeline fails as a whole (no device, no library, a batch error) still
    joins every collective, with no results; the failure is agreed (MAX over ranks), nothing
    is published and every rank exits 1.  Per-tensor failures are skipped and logged as in
    the single-process CLI."""
    backend = os.environ.get("AWQ_DIST_BACKEND", "nccl")      # gloo: tests with 2 ranks on one GPU
    if backend != "nccl":
        D.init(backend)
    rank, local, world = D.init("nccl") if backend == "nccl" else D.env_world()
    device = f"cuda:{local % max(1, torch.cuda.device_count())}"
    comm = torch.device(device) if backend == "nccl" else torch.device("cpu")
    owner = dict(zip((i.name for i in ordered), D.shard([i.nbytes for i in ordered], world)))
    mine = [i for i in ordered if owner[i.name] == rank]
    autoawq = cfg.export_autoawq
    per_rank = args.dist_output == "per_rank"
    if per_rank and not _shared_output_dir(args.output_dir, rank, world, logger):
        # node-local disks (multi-node torchrun): rank 0's metadata.json could not reach the
        # other ranks' chunk files, so every result goes to rank 0 instead
        if rank == 0:
            logger.warning(f"{args.output_dir} is not one shared directory for all {world} ranks; "
                           f"falling back to --dist_output gather")
        per_rank = False
    results: Dict[str, Dict[str, torch.Tensor]] = {}
    writer, failed = None, 0
    t0 = time.time()
    try:
        q = new_quantizer(args, device)
        logger.info(f"rank {rank}/{world}: {len(mine)} of {len(ordered)} tensors on {device}")
        if per_rank and not autoawq:
            writer = ChunkWriter([i.name for i in mine], args.output_dir, args.chunk_size, args.save_safetensors,
                                 logger, stem=_rank_stem(rank), metadata=False,
                                 writers=writer_threads(mine, cfg.packed))
        # per-rank chunks: the writer holds each result until its chunk is on disk, nothing else does
        sink = _NullSink() if writer is not None else results
        pipeline.quantize_stream(replace(cfg, keep_on_device=not per_rank), loader, mine, q, device, sink,
                                 threading.Lock(), logger, on_done=writer.done if writer else None, writer=writer)
    except Exception as e:  # noqa: BLE001  (agreed below: every rank exits 1)
        logger.error(f"rank {rank}: quantization failed: {e}")
        failed = 1
    if writer is not None:
        try:
            writer.close()
        except Exception as e:  # noqa: BLE001
            logger.error(f"rank {rank}: writing chunks failed: {e}")
            failed = 1
    if failed:
        results = {}
    TIMINGS[f"rank{rank}_quantize_write_s"] = round(time.time() - t0, 4)
    try:
        if per_rank and autoawq:
            rc = _commit_rank_autoawq(args, loader, ordered, mine, results, passthrough or [], rank, world, failed,
                                      comm, logger)
        elif per_rank:
            rc = _commit_rank_chunks(args, ordered, writer, rank, world, failed, comm, logger)
        else:
            rc = _gather_and_write(args, loader, ordered, results, passthrough or [], rank, world, failed, comm,
                                   logger)
    finally:
        dist.destroy_process_group()
    if rank == 0 and rc == 0:
        return finish_run(args, ordered, {i.name for i in ordered}, logger, start, world=world)
    return rc


def _shared_output_dir(output_dir: str, rank: int, world: int, logger) -> bool:
    """True if every rank sees the same output directory (per-rank chunk files are only a
    checkpoint when rank 0's metadata.json and every rank's chunks land in one directory):
    rank 0 creates a sentinel file with a random name, every rank looks for it."""
    import secrets
    token = [secrets.token_hex(8) if rank == 0 else None]
    dist.broadcast_object_list(token, src=0)
    path = os.path.join(output_dir, f".awq_shared_{token[0]}")
    made = 1
    if rank == 0:
        try:
            os.makedirs(output_dir, exist_ok=True)
            with open(path, "w") as f:
                f.write("awq_quantizer per-rank output check\n")
        except OSError as e:
            logger.error(f"cannot write to {output_dir}: {e}")
            made = 0
    dist.barrier()
    seen = [None] * world
    dist.all_gather_object(seen, bool(made) and os.path.exists(path))
    dist.barrier()
    if rank == 0 and made:
        try:
            os.remove(path)
        except OSError:
            pass
    return all(seen)


def _agree(flag: int, comm: torch.device) -> int:
    """MAX of a per-rank int over all ranks (a failure anywhere fails everyone)."""
    return int(D.max_over_ranks(float(flag), comm))


def _remove_rank_files(output_dir: str, rank: int, also: List[str] = ()) -> None:
    """Nothing is published: remove every chunk file under this rank's private stem, whatever
    its state, and `also` (the files it had already renamed)."""
    tmp = _rank_stem(rank).split("{")[0]
    for f in list(also) + [os.path.join(output_dir, f) for f in os.listdir(output_dir) if f.startswith(tmp)]:
        try:
            os.remove(f)
        except OSError:
            pass


def _commit_rank_chunks(args, ordered: List[TensorInfo], writer: Optional[ChunkWriter], rank: int, world: int,
                        failed: int, comm: torch.device, logger) -> int:
    """Per-rank chunk files -> the reference layout: global chunk numbers in rank order,
    metadata.json (rank 0) whose tensor_to_chunk lists every tensor in processing order.
    Loading the chunks through metadata.json gives exactly the single-process result dicts
    (tests/test_dist_output.py)."""
    st = args.save_safetensors
    mine = {"failed": failed, "t2c": dict(writer.t2c) if writer and not failed else {},
            "n_chunks": writer.n_chunks if writer and not failed else 0,
            "qparams": writer.qparams if writer and not failed else None}
    infos = [None] * world
    dist.all_gather_object(infos, mine)
    n_own = mine["n_chunks"]
    if any(i["failed"] for i in infos):
        _remove_rank_files(args.output_dir, rank)
        if rank == 0:
            logger.error("A rank failed; no output was published")
        return 1
    offs = [0] * world
    for r in range(1, world):
        offs[r] = offs[r - 1] + infos[r - 1]["n_chunks"]
    bad = 0
    renamed = []
    try:
        for c in range(n_own):
            dst = _chunk_path(args.output_dir, offs[rank] + c, st)
            os.replace(_chunk_path(args.output_dir, c, st, _rank_stem(rank)), dst)
            renamed.append(dst)
    except OSError as e:
        logger.error(f"rank {rank}: renaming chunk files failed: {e}")
        bad = 1
    rc = _agree(bad, comm)
    if rank == 0 and rc == 0:
        t2c = {}
        for info in ordered:           # processing order = bytes descending (main.py:259)
            for r, i in enumerate(infos):
                if info.name in i["t2c"]:
                    t2c[info.name] = offs[r] + i["t2c"][info.name]
                    break
        total = offs[-1] + infos[-1]["n_chunks"]
        if not t2c:
            logger.error("No tensors were successfully quantized")
            rc = 1
        else:
            qparams = next(i["qparams"] for i in infos if i["qparams"] is not None)
            try:
                _write_metadata(args.output_dir, total, args.chunk_size, t2c, st, len(t2c), qparams, logger)
                logger.info(f"Successfully quantized {len(t2c)} tensors on {world} GPUs; {total} chunk files "
                            f"written by their ranks")
            except OSError as e:
                logger.error(f"Failed to save quantized model: {e}")
                rc = 1
    rc = _agree(rc, comm)
    if rc:
        _remove_rank_files(args.output_dir, rank, also=renamed)
    return rc


def _commit_rank_autoawq(args, loader, ordered: List[TensorInfo], mine: List[TensorInfo],
                         results: Dict[str, Dict[str, torch.Tensor]], passthrough: List[TensorInfo], rank: int,
                         world: int, failed: int, comm: torch.device, logger) -> int:
    """AutoAWQ checkpoint written by its ranks: rank r writes its quantized linears (and its
    linears that failed, unquantized) as one safetensors shard, rank 0 adds the passthrough
    tensors, and rank 0 writes model.safetensors.index.json (the transformers sharded-
    checkpoint index) plus the configs.  One rank with tensors writes model.safetensors."""
    from safetensors.torch import save_file
    not_quant = [i for i in mine if i.name not in results]
    has = bool(results or not_quant or (rank == 0 and passthrough))
    flags = [None] * world
    dist.all_gather_object(flags, {"failed": failed, "has": has, "n_ok": len(results)})
    if any(f["failed"] for f in flags):
        if rank == 0:
            logger.error("A rank failed; no output was published")
        return 1
    if sum(f["n_ok"] for f in flags) == 0:
        if rank == 0:
            logger.error("No tensors were successfully quantized")
        return 1
    writers = [r for r in range(world) if flags[r]["has"]]
    fname = ("model.safetensors" if len(writers) == 1 else
             f"model-{writers.index(rank) + 1:05d}-of-{len(writers):05d}.safetensors") if has else None
    keys, size, bad = [], 0, 0
    if has:
        try:
            tensors = autoawq_tensors(results, loader, passthrough if rank == 0 else [], not_quant)
            save_file(tensors, os.path.join(args.output_dir, fname), metadata={"format": "pt"})
            keys = list(tensors)
            size = sum(t.numel() * t.element_size() for t in tensors.values())
        except Exception as e:  # noqa: BLE001
            logger.error(f"rank {rank}: writing {fname} failed: {e}")
            bad = 1
    shards = [None] * world
    dist.all_gather_object(shards, {"file": fname, "keys": keys, "size": size, "bad": bad,
                                    "not_converted": [i.name[: -len(".weight")] for i in not_quant]})

    def unpublish():   # nothing is published: every rank removes the shard it wrote
        if fname and os.path.exists(os.path.join(args.output_dir, fname)):
            try:
                os.remove(os.path.join(args.output_dir, fname))
            except OSError:
                pass
    if any(s["bad"] for s in shards):
        unpublish()
        return 1
    rc = 0
    if rank == 0:
        try:
            if len(writers) > 1:
                wmap = {k: s["file"] for s in shards for k in s["keys"]}
                index = {"metadata": {"total_size": sum(s["size"] for s in shards)},
                         "weight_map": {k: wmap[k] for k in sorted(wmap)}}
                with open(os.path.join(args.output_dir, "model.safetensors.index.json"), "w") as f:
                    json.dump(index, f, indent=2)
            order = {i.name[: -len(".weight")]: k for k, i in enumerate(ordered)}
            nc = sorted((m for s in shards for m in s["not_converted"]), key=lambda m: order.get(m, 0))
            write_autoawq_configs(args.output_dir, args, loader, nc, logger)
            logger.info(f"Saved AutoAWQ checkpoint from {world} ranks: {sum(f['n_ok'] for f in flags)} quantized "
                        f"linear weights in {len(writers)} shard file(s)")
        except Exception as e:  # noqa: BLE001
            logger.error(f"Failed to save quantized model: {e}")
            rc = 1
    rc = _agree(rc, comm)
    if rc:
        unpublish()
    return rc


def _gather_and_write(args, loader, ordered: List[TensorInfo], results: Dict[str, Dict[str, torch.Tensor]],
                      passthrough: List[TensorInfo], rank: int, world: int, failed: int, comm: torch.device,
                      logger) -> int:
    """--dist_output gather: the packed results of every rank go to rank 0 in one batched
    point-to-point round (distributed.gather_to_rank0), rank 0 writes the single-process
    layout."""
    autoawq = args.output_format == "autoawq"
    # which tensors succeeded, and the shapes rank 0 must receive (tiny metadata)
    meta = {n: {f: (tuple(t.shape), str(t.dtype)) for f, t in r.items() if f not in _SCALARS}
            for n, r in results.items()}
    all_meta = [None] * world
    dist.all_gather_object(all_meta, {"failed": failed, "meta": meta})
    if any(m["failed"] for m in all_meta):
        if rank == 0:
            logger.error("A rank failed; no output was published")
        return 1
    ok_owner, shapes = {}, {}
    for r, m in enumerate(all_meta):
        for n, fields in m["meta"].items():
            ok_owner[n] = r
            shapes[n] = {f: (shp, getattr(torch, dt.split(".")[-1])) for f, (shp, dt) in fields.items()}
    payload = {n: {f: t.to(comm) for f, t in r.items() if f not in _SCALARS} for n, r in results.items()}
    merged = D.gather_to_rank0(payload, ok_owner, shapes, comm)
    rc = 0
    if rank == 0:
        scal = {"bits": torch.tensor(args.bits, dtype=torch.int32),
                "group_size": torch.tensor(args.group_size, dtype=torch.int32),
                "symmetric": torch.tensor(args.symmetric, dtype=torch.bool)}
        quantized = {}
        for info in ordered:
            if info.name in merged:
                d = _to_cpu(merged[info.name])
                if not autoawq:
                    d.update(scal)
                if args.output_format == "packed":
                    d["shape"] = torch.tensor(list(info.shape), dtype=torch.int64)
                quantized[info.name] = d
        if not quantized:
            logger.error("No tensors were successfully quantized")
            rc = 1
        else:
            logger.info(f"Successfully quantized {len(quantized)} tensors on {world} GPUs")
            try:
                if autoawq:
                    save_autoawq(quantized, loader, passthrough, args.output_dir, args, logger,
                                 failed=[i for i in ordered if i.name not in quantized])
                else:
                    save_model_in_chunks(quantized, args.output_dir, chunk_size=args.chunk_size,
                                         use_safetensors=args.save_safetensors, logger=logger)
            except Exception as e:  # noqa: BLE001
                logger.error(f"Failed to save quantized model: {e}")
                rc = 1
    return _agree(rc, comm)
