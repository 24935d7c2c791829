"""The awq_quantizer CLI (drop-in for reference src/awq_quantizer/main.py).

CPU tests: flag surface and defaults (reference main.py:22-159), tensor filter and order
(main.py:241-259), LPT partition (main.py:395-427), output layout (main.py:430-512), exit
codes.  GPU test: end-to-end run on a small safetensors model, every result equal to the
oracle."""
import json
import os
import sys

import pytest
import torch
from safetensors.torch import load_file, save_file


def test_defaults_match_reference_cli():
    from awq_quantizer.main import parse_args
    a = parse_args(["--model_id", "m", "--output_dir", "o"])
    assert (a.bits, a.group_size, a.symmetric, a.zero_point, a.percentile, a.scale_method, a.per_channel) == \
        (4, 128, False, "minmax", 0.99, "mse", False)
    assert (a.num_workers, a.max_memory, a.multi_gpu, a.batch_size, a.prefetch_factor, a.memory_efficient) == \
        (4, 0.8, False, 10, 2, False)
    assert (a.log_level, a.log_file, a.save_safetensors, a.chunk_size) == ("INFO", None, False, 10)
    assert a.device == ("cuda" if torch.cuda.is_available() else "cpu")
    with pytest.raises(SystemExit):
        parse_args(["--model_id", "m", "--output_dir", "o", "--bits", "3"])
    with pytest.raises(SystemExit):
        parse_args(["--output_dir", "o"])


def _model_dir(tmp_path, tensors, files=1):
    d = tmp_path / "model"
    d.mkdir()
    names = list(tensors)
    per = -(-len(names) // files)
    for i in range(files):
        part = {n: tensors[n] for n in names[i * per:(i + 1) * per]}
        if part:
            save_file(part, str(d / f"model-{i:05d}-of-{files:05d}.safetensors"))
    return str(d)


def _tensors():
    g = torch.Generator().manual_seed(0)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.02).to(torch.bfloat16)
    return {
        "model.embed.weight": r(300, 256),
        "model.layers.0.mlp.fc1.weight": r(256, 768),
        "model.layers.0.mlp.fc1.bias": r(768),
        "model.layers.0.ln.weight": torch.ones(256, dtype=torch.bfloat16),
        "model.layers.0.attn.qkv.weight": r(96, 3, 64),
        "model.layers.0.small": r(10, 10),
        "model.layers.0.int": torch.arange(300, dtype=torch.int32),
        "model.layers.0.fp16.weight": r(64, 256).to(torch.float16),
    }


def test_select_order_and_partition(tmp_path):
    from awq_quantizer.main import partition_tensors, select_tensors
    from awq_quantizer.model_loading import load_model_from_path
    loader = load_model_from_path(_model_dir(tmp_path, _tensors(), files=2), logger_level="ERROR")
    sel = select_tensors(loader.tensor_index())
    names = [i.name for i in sel]
    assert "model.layers.0.small" not in names and "model.layers.0.int" not in names   # numel<128, not float
    sizes = [i.nbytes for i in sel]
    assert sizes == sorted(sizes, reverse=True)
    parts = partition_tensors(sel, 3)
    assert sorted(i.name for p in parts for i in p) == sorted(names)
    loads = [sum(i.nbytes for i in p) for p in parts]
    assert max(loads) - min(loads) <= max(sizes)          # greedy LPT balance bound


def test_batch_budget_and_batches(monkeypatch):
    """About 8 pipeline batches per model (32 MiB floor, batch_bytes cap); processing order
    kept; a tensor larger than the budget is a batch of its own."""
    from awq_quantizer.main import _batch_budget, _batches
    from awq_quantizer.model_loading.safetensors_loader import TensorInfo
    MiB = 1 << 20
    assert _batch_budget(662 * MiB, 1 << 30) == 662 * MiB // 8        # opt-350m: ~83 MB batches
    assert _batch_budget(100 * MiB, 1 << 30) == 32 * MiB               # floor
    assert _batch_budget(16 << 30, 1 << 30) == 1 << 30                 # Llama-3-8B: the cap
    infos = [TensorInfo(f"t{i}", "f", torch.bfloat16, (n,)) for i, n in enumerate([10, 20, 100, 5, 5, 30])]
    bs = _batches(infos, 60)                                           # bytes: 20 40 200 10 10 60
    assert [[i.name for i in b] for b in bs] == [["t0", "t1"], ["t2"], ["t3", "t4"], ["t5"]]


def test_save_layout(tmp_path):
    from awq_quantizer.main import save_model_in_chunks
    res = {f"t{i}": {"tensor_q": torch.zeros(4, 8, dtype=torch.int32), "scales": torch.ones(4, 1, dtype=torch.float16),
                     "zero_points": torch.zeros(4, 1, dtype=torch.int32), "bits": torch.tensor(4, dtype=torch.int32),
                     "group_size": torch.tensor(128, dtype=torch.int32), "symmetric": torch.tensor(False)}
           for i in range(5)}
    save_model_in_chunks(res, str(tmp_path / "pt"), chunk_size=2)
    meta = json.load(open(tmp_path / "pt" / "metadata.json"))
    assert meta["num_chunks"] == 3 and meta["num_tensors"] == 5 and meta["format"] == "pytorch"
    assert meta["tensor_to_chunk"] == {"t0": 0, "t1": 0, "t2": 1, "t3": 1, "t4": 2}
    assert meta["quantization_params"] == {"bits": 4, "group_size": 128, "symmetric": False}
    chunk = torch.load(str(tmp_path / "pt" / "model_chunk_0001.pt"), weights_only=True)
    assert set(chunk) == {"t2", "t3"} and torch.equal(chunk["t2"]["tensor_q"], res["t2"]["tensor_q"])
    save_model_in_chunks(res, str(tmp_path / "st"), chunk_size=10, use_safetensors=True)   # works (reference: fails)
    from safetensors.torch import load_file
    flat = load_file(str(tmp_path / "st" / "model_chunk_0000.safetensors"))
    assert "t4.tensor_q" in flat and json.load(open(tmp_path / "st" / "metadata.json"))["format"] == "safetensors"


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU exit code")
@pytest.mark.parametrize("use_st", [False, True])
def test_chunk_writer_matches_serial_save(tmp_path, use_st):
    """ChunkWriter (chunks written while the pipeline runs, out-of-order completions from
    several threads, some tensors failing) produces exactly save_model_in_chunks' files."""
    import random
    import threading
    from safetensors.torch import load_file
    from awq_quantizer.main import ChunkWriter, save_model_in_chunks
    order = [f"layer.{i}.weight" for i in range(23)]
    failed = {order[3], order[10], order[11]}
    res = {n: {"qweight": torch.full((4, 2), i, dtype=torch.int32), "scales": torch.full((4, 1), i, dtype=torch.float16),
               "bits": torch.tensor(4, dtype=torch.int32), "group_size": torch.tensor(128, dtype=torch.int32),
               "symmetric": torch.tensor(False)} for i, n in enumerate(order)}
    w = ChunkWriter(order, str(tmp_path / "a"), 5, use_st, writers=3)
    names = order[:]
    random.Random(0).shuffle(names)
    ths = [threading.Thread(target=lambda part: [w.done(n, None if n in failed else res[n]) for n in part],
                            args=(names[k::3],)) for k in range(3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    w.close()
    ok = {n: res[n] for n in order if n not in failed}
    save_model_in_chunks(ok, str(tmp_path / "b"), chunk_size=5, use_safetensors=use_st)
    a_files, b_files = sorted(os.listdir(tmp_path / "a")), sorted(os.listdir(tmp_path / "b"))
    assert a_files == b_files and len(a_files) == 5          # 20 tensors -> 4 chunks + metadata
    assert json.load(open(tmp_path / "a" / "metadata.json")) == json.load(open(tmp_path / "b" / "metadata.json"))
    for f in a_files:
        if f.endswith(".pt"):
            x, y = torch.load(tmp_path / "a" / f, weights_only=True), torch.load(tmp_path / "b" / f, weights_only=True)
            assert list(x) == list(y) and all(torch.equal(x[n][k], y[n][k]) for n in x for k in x[n])
        elif f.endswith(".safetensors"):
            x, y = load_file(str(tmp_path / "a" / f)), load_file(str(tmp_path / "b" / f))
            assert list(x) == list(y) and all(torch.equal(x[k], y[k]) for k in x)


def test_chunk_writer_close_marks_unfinished_failed(tmp_path):
    from awq_quantizer.main import ChunkWriter
    order = ["a", "b", "c"]
    w = ChunkWriter(order, str(tmp_path), 2, False, writers=1)
    w.done("a", {"q": torch.zeros(1), "bits": torch.tensor(4)})
    w.close()                      # "b", "c" never reported (a device worker died): skipped
    meta = json.load(open(tmp_path / "metadata.json"))
    assert meta["num_tensors"] == 1 and meta["tensor_to_chunk"] == {"a": 0}


def test_cpu_share_reads_cgroup_quota(monkeypatch, tmp_path):
    """cpu_share: the affinity set, capped by a cgroup v2 quota (the GPU box: cpu.max 1600000
    100000 = 16 CPUs while os.cpu_count() shows the node's 256)."""
    import builtins
    from awq_quantizer import output as m
    real_open = builtins.open
    monkeypatch.setattr(m.os, "sched_getaffinity", lambda pid: set(range(256)), raising=False)

    def fake_open(path, *a, **k):
        if path == "/sys/fs/cgroup/cpu.max":
            q = tmp_path / "cpu.max"
            q.write_text(quota)
            return real_open(q, *a, **k)
        return real_open(path, *a, **k)
    monkeypatch.setattr(builtins, "open", fake_open)
    quota = "1600000 100000\n"
    assert m.cpu_share() == 16
    quota = "max 100000\n"
    assert m.cpu_share() == 256
    quota = "50000 100000\n"
    assert m.cpu_share() == 1


def test_writer_threads_by_output_size(monkeypatch):
    """Chunk-writer pool sized by output bytes: 2-4 writers below ~2 GB of output (more
    stalled the pipeline's HIP calls), up to 8 above; STREAM_OPTS["writers"] overrides."""
    from awq_quantizer import output as m
    from awq_quantizer.model_loading.safetensors_loader import TensorInfo
    monkeypatch.setattr(m, "cpu_share", lambda: 16)

    def infos(total):
        return [TensorInfo("w", "f", torch.bfloat16, (total // 2,))]
    assert m.writer_threads(infos(662 << 20), packed=True) == 4          # opt-350m packed
    assert m.writer_threads(infos(662 << 20), packed=False) == 4         # ~1.3 GB reference output
    assert m.writer_threads(infos(16 << 30), packed=True) == 8           # Llama-3-8B packed: 4.2 GB out
    monkeypatch.setattr(m, "cpu_share", lambda: 4)
    assert m.writer_threads(infos(16 << 30), packed=False) == 2
    monkeypatch.setitem(m.STREAM_OPTS, "writers", 3)
    assert m.writer_threads(infos(16 << 30), packed=True) == 3


def test_chunk_writer_widens_pool_at_close(tmp_path, monkeypatch):
    """While producers run at most `writers` chunk writes run at once; once every tensor has
    reported (or at close()) the rest of the pool drains the backlog (same files either way)."""
    import threading
    import time as _t
    from awq_quantizer import output as m
    monkeypatch.setattr(m, "cpu_share", lambda: 16)          # tail pool: 8
    active, peak, lock = [0], [0], threading.Lock()
    real = m._write_chunk

    def slow_write(*a, **k):
        with lock:
            active[0] += 1
            peak[0] = max(peak[0], active[0])
        _t.sleep(0.05)
        real(*a, **k)
        with lock:
            active[0] -= 1
    monkeypatch.setattr(m, "_write_chunk", slow_write)
    order = [f"t{i}" for i in range(16)]
    w = m.ChunkWriter(order, str(tmp_path), 1, False, writers=2)
    for n in order[:-1]:
        w.done(n, {"q": torch.zeros(2), "bits": torch.tensor(4)})
    _t.sleep(0.12)
    assert peak[0] <= 2                                      # gated while "producing"
    w.done(order[-1], {"q": torch.zeros(2), "bits": torch.tensor(4)})   # the last report widens
    _t.sleep(0.12)
    assert peak[0] > 2                                       # the backlog drains wider
    w.close()
    assert json.load(open(tmp_path / "metadata.json"))["num_chunks"] == 16


def test_loader_read_into_matches_safetensors(tmp_path):
    """read_into (pread at the header offsets, the CLI's pinned-read path) == safetensors'
    own read for every dtype, empty tensors and several files."""
    from awq_quantizer.model_loading import load_model_from_path
    t = {"a": torch.randn(37, 129).to(torch.bfloat16), "b": torch.arange(10, dtype=torch.int32),
         "c": torch.randn(5).half(), "d": torch.randn(3, 4, 5), "e": torch.zeros(0, 3), "f": torch.randn(7).double()}
    loader = load_model_from_path(_model_dir(tmp_path, t, files=2), logger_level="ERROR")
    for info in loader.tensor_index():
        out = torch.empty(info.shape, dtype=info.dtype)
        assert torch.equal(loader.read_into(info, out), t[info.name]), info.name
        assert torch.equal(out, loader.read(info)), info.name
    with pytest.raises(ValueError, match="header size"):
        info = [i for i in loader.tensor_index() if i.name == "a"][0]
        loader.read_into(info, torch.empty(36, 129, dtype=torch.bfloat16))
    loader.close()


def test_main_without_gpu_returns_1(tmp_path):
    from awq_quantizer.main import main
    d = _model_dir(tmp_path, _tensors())
    assert main(["--model_id", d, "--output_dir", str(tmp_path / "out"), "--log_level", "CRITICAL"]) == 1


def test_main_missing_model_returns_1(tmp_path):
    from awq_quantizer.main import main
    assert main(["--model_id", str(tmp_path / "nope"), "--output_dir", str(tmp_path / "out"),
                 "--log_level", "CRITICAL"]) == 1


def _load_chunk(out, ci, st):
    if st:
        flat = load_file(str(out / f"model_chunk_{ci:04d}.safetensors"))
        res = {}
        for k, v in flat.items():
            name, field = k.rsplit(".", 1)
            res.setdefault(name, {})[field] = v
        return res
    return torch.load(str(out / f"model_chunk_{ci:04d}.pt"), weights_only=True)


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")
@pytest.mark.parametrize("fmt", ["reference", "packed"])
@pytest.mark.parametrize("engine,st", [("native", False), ("native", True), ("python", False)])
def test_main_end_to_end_gpu(tmp_path, fmt, engine, st):
    from oracle import awq_oracle as orc
    from awq_quantizer.main import main
    tensors = _tensors()
    d = _model_dir(tmp_path, tensors, files=2)
    out = tmp_path / "out"
    rc = main(["--model_id", d, "--output_dir", str(out), "--log_level", "ERROR", "--chunk_size", "3",
               "--output_format", fmt, "--stream_engine", engine] + (["--save_safetensors"] if st else []))
    assert rc == 0
    meta = json.load(open(out / "metadata.json"))
    assert meta["num_tensors"] == 6
    for name, chunk_idx in meta["tensor_to_chunk"].items():
        res = _load_chunk(out, chunk_idx, st)[name]
        ref = orc.quantize(tensors[name], bits=4, group_size=128, symmetric=False, per_channel=False)
        if fmt == "reference":
            assert torch.equal(res["tensor_q"], ref["tensor_q"]), name
            assert torch.equal(res["zero_points"], ref["zero_points"]), name
            assert torch.equal(res["scales"].view(torch.int16), ref["scales"].view(torch.int16)), name
        else:
            rows = 1 if tensors[name].dim() <= 1 else tensors[name].shape[0]
            assert torch.equal(res["qweight"], orc.pack_rows(ref["tensor_q"].reshape(rows, -1), 4, 0)), name
            assert torch.equal(res["qzeros"], orc.pack_rows(ref["zero_points"], 4, 0)), name


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")
@pytest.mark.parametrize("mode", ["per_rank", "gather"])
def test_main_torchrun_two_ranks_gpu(tmp_path, mode):
    """torchrun, 2 ranks sharing the box's GPU (gloo for the collectives: RCCL refuses two
    ranks on one device); per_rank: each rank writes its chunks, gather: rank 0 writes
    everything — either way every tensor, equal to the oracle, through metadata.json."""
    import socket
    import subprocess
    import sys
    from oracle import awq_oracle as orc
    tensors = _tensors()
    d = _model_dir(tmp_path, tensors, files=2)
    out = tmp_path / "out"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AWQ_DIST_BACKEND="gloo",
               PYTHONPATH=os.pathsep.join([os.path.join(root, "awq-converter_amd"), root]))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", "-m", "awq_quantizer.main",
           "--model_id", d, "--output_dir", str(out), "--log_level", "ERROR", "--output_format", "packed",
           "--dist_output", mode, "--chunk_size", "2"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    meta = json.load(open(out / "metadata.json"))
    assert meta["num_tensors"] == 6
    for name, ci in meta["tensor_to_chunk"].items():
        res = torch.load(str(out / f"model_chunk_{ci:04d}.pt"), weights_only=True)[name]
        ref = orc.quantize(tensors[name], bits=4, group_size=128, symmetric=False)
        rows = 1 if tensors[name].dim() <= 1 else tensors[name].shape[0]
        assert torch.equal(res["qweight"], orc.pack_rows(ref["tensor_q"].reshape(rows, -1), 4, 0)), name
        assert torch.equal(res["scales"].view(torch.int16), ref["scales"].view(torch.int16)), name


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")
def test_main_fresh_process_early_warmup_gpu(tmp_path):
    """`python -m awq_quantizer.main` as users run it: a fresh process, where main() starts
    the device's first-use warm-up (awq_runtime_warmup) before indexing and the pipeline
    joins it — every tensor equal to the oracle; the INFO device line names the GPU."""
    import subprocess
    import sys
    from oracle import awq_oracle as orc
    tensors = _tensors()
    d = _model_dir(tmp_path, tensors, files=2)
    out = tmp_path / "out"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "awq-converter_amd"), root]))
    r = subprocess.run([sys.executable, "-m", "awq_quantizer.main", "--model_id", d, "--output_dir", str(out),
                        "--output_format", "packed", "--chunk_size", "2"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"Using GPU cuda: {torch.cuda.get_device_name(0)}" in r.stdout or \
        f"Using GPU cuda:0: {torch.cuda.get_device_name(0)}" in r.stdout, r.stdout[-2000:]
    meta = json.load(open(out / "metadata.json"))
    assert meta["num_tensors"] == 6
    for name, ci in meta["tensor_to_chunk"].items():
        res = torch.load(str(out / f"model_chunk_{ci:04d}.pt"), weights_only=True)[name]
        ref = orc.quantize(tensors[name], bits=4, group_size=128, symmetric=False)
        rows = 1 if tensors[name].dim() <= 1 else tensors[name].shape[0]
        assert torch.equal(res["qweight"], orc.pack_rows(ref["tensor_q"].reshape(rows, -1), 4, 0)), name
        assert torch.equal(res["scales"].view(torch.int16), ref["scales"].view(torch.int16)), name


def test_warmup_api_without_gpu():
    """awq_runtime_warmup_wait for a device never warmed returns at once; bad indices fail."""
    from awq_quantizer import _hip
    import ctypes
    lib = _hip.load_library()
    secs = ctypes.c_double(-1.0)
    assert lib.awq_runtime_warmup_wait(3, ctypes.byref(secs)) == 0 and secs.value == 0.0
    assert lib.awq_runtime_warmup(-1) != 0 and lib.awq_runtime_warmup(64) != 0
    assert lib.awq_runtime_warmup_wait(64, None) != 0


def test_early_warmup_device_from_argv(monkeypatch):
    """_early.device_index: the CLI's one GPU from its arguments alone, None whenever it
    cannot be sure (CPU, several devices, torchrun, an abbreviated option)."""
    from awq_quantizer._early import device_index
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert device_index([]) == 0 and device_index(["--model_id", "m", "--output_dir", "o"]) == 0
    assert device_index(["--device", "cuda:3"]) == 3 and device_index(["--device=cuda:1"]) == 1
    for argv in (["--device", "cpu"], ["--device", "all"], ["--multi_gpu"], ["--dev", "cuda:1"],
                 ["--device", "cuda:x"]):
        assert device_index(argv) is None, argv
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert device_index([]) is None


def test_console_entry_starts_warmup_before_torch(tmp_path):
    """The `awq_quantizer` console script (awq_quantizer.cli:run) imports neither torch nor the
    CLI module before _early.start has run; on a missing model it exits 1 like main()."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.path.join(root, "awq-converter_amd"))
    code = ("import sys\n"
            "from awq_quantizer import _early\n"
            "real = _early.start\n"
            "def spy(argv):\n"
            "    assert 'torch' not in sys.modules and 'awq_quantizer.main' not in sys.modules\n"
            "    print('EARLY', argv)\n"
            "    return real(argv)\n"
            "_early.start = spy\n"
            "sys.argv = ['awq_quantizer', '--model_id', sys.argv[1], '--output_dir', sys.argv[2]]\n"
            "from awq_quantizer.cli import run\n"
            "run()\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "missing"), str(tmp_path / "out")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert "EARLY ['--model_id'" in r.stdout


def test_linear_selection_for_autoawq():
    from awq_quantizer.main import is_linear_weight
    from awq_quantizer.model_loading import TensorInfo
    mk = lambda n, s, dt=torch.bfloat16: TensorInfo(n, "f", dt, s)
    assert is_linear_weight(mk("model.layers.0.mlp.fc1.weight", (256, 768)), 128)
    assert not is_linear_weight(mk("model.embed_tokens.weight", (512, 256)), 128)
    assert not is_linear_weight(mk("lm_head.weight", (512, 256)), 128)
    assert not is_linear_weight(mk("model.layers.0.ln.weight", (256,)), 128)
    assert not is_linear_weight(mk("model.layers.0.x.weight", (250, 256)), 128)      # out % 8
    assert not is_linear_weight(mk("model.layers.0.x.weight", (256, 200)), 128)      # in % group
    assert not is_linear_weight(mk("model.layers.0.x.bias", (256, 256)), 128)
    # MoE routers stay fp16 (AutoAWQ); gate_proj is a linear
    assert not is_linear_weight(mk("model.layers.0.block_sparse_moe.gate.weight", (8, 4096)), 128)
    assert not is_linear_weight(mk("model.layers.0.mlp.gate.weight", (64, 2048)), 128)
    assert not is_linear_weight(mk("model.layers.0.mlp.router.weight", (64, 2048)), 128)
    assert is_linear_weight(mk("model.layers.0.mlp.gate_proj.weight", (14336, 4096)), 128)
    assert is_linear_weight(mk("model.layers.0.block_sparse_moe.experts.0.w1.weight", (14336, 4096)), 128)
    # GPT-2 Conv1D weights are [in, out]: never quantized as linears
    assert not is_linear_weight(mk("h.0.attn.c_attn.weight", (768, 2304)), 128, "gpt2")
    for mt in ("openai-gpt", "imagegpt", "decision_transformer"):   # other Conv1D [in, out] models
        assert not is_linear_weight(mk("h.0.attn.c_attn.weight", (768, 2304)), 128, mt), mt
    assert is_linear_weight(mk("h.0.attn.c_attn.weight", (768, 2304)), 128, "llama")


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")
def test_main_autoawq_output_gpu(tmp_path):
    from safetensors.torch import load_file
    from oracle import awq_oracle as orc
    from awq_quantizer.main import main
    tensors = _tensors()
    d = _model_dir(tmp_path, tensors, files=2)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"model_type": "opt", "hidden_size": 256}, f)
    out = tmp_path / "out"
    assert main(["--model_id", d, "--output_dir", str(out), "--log_level", "ERROR", "--output_format", "autoawq"]) == 0
    st = load_file(str(out / "model.safetensors"))
    for name in ("model.layers.0.mlp.fc1.weight", "model.layers.0.fp16.weight"):
        prefix = name[: -len(".weight")]
        ref = orc.quantize(tensors[name], bits=4, group_size=128, symmetric=False)
        qw, qz, sc = orc.autoawq_pack(ref["tensor_q"].to(torch.int64), ref["zero_points"].to(torch.int64),
                                      ref["scales"])
        assert torch.equal(st[prefix + ".qweight"], qw) and torch.equal(st[prefix + ".qzeros"], qz), name
        assert torch.equal(st[prefix + ".scales"], sc), name
        assert name not in st
    for name in ("model.embed.weight", "model.layers.0.mlp.fc1.bias", "model.layers.0.ln.weight",
                 "model.layers.0.attn.qkv.weight", "model.layers.0.small", "model.layers.0.int"):
        assert torch.equal(st[name], tensors[name]), name
    qc = json.load(open(out / "quant_config.json"))
    assert qc == {"zero_point": True, "q_group_size": 128, "w_bit": 4, "version": "GEMM"}
    cfg = json.load(open(out / "config.json"))
    assert cfg["quantization_config"]["quant_method"] == "awq" and cfg["model_type"] == "opt"
    assert main(["--model_id", d, "--output_dir", str(tmp_path / "o8"), "--log_level", "CRITICAL", "--bits", "8",
                 "--output_format", "autoawq"]) == 1


@pytest.mark.gpu
def test_bench_two_ranks_gpu():
    """bench.py's N>1 path (max-over-ranks timing, the gather leg) with 2 ranks on the box's
    one GPU over gloo; the driver runs it over RCCL, one rank per GPU."""
    import socket
    import subprocess
    import sys
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AWQ_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(root, "bench.py"), "--gpus", "2",
           "--steps", "3", "--warmup", "1", "--workload", "c1", "--replica", "--no-cpu-baseline", "--no-copy-ceiling"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["scaling"] == "weak"
    # one peer's packed outputs of the 1024x4096 tensor: qweight 2 MiB + qzeros 16 KiB + scales 64 KiB
    assert line["exchange"]["bytes_to_rank0"] == 1024 * 512 * 4 + 1024 * 4 * 4 + 1024 * 32 * 2
    assert line["exchange"]["ms"] > 0


@pytest.mark.gpu
def test_bench_two_ranks_shard_gpu(tmp_path):
    """bench.py --shard (strong scaling: the opt-125m tensor list LPT-sharded over 2 ranks,
    gloo on the box's one GPU): value counts the set once, the gather moves exactly the peer's
    packed shard (derived here from distributed.shard and the packed output shapes)."""
    import socket
    import subprocess
    import sys
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    from awq_quantizer import distributed as D
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, AWQ_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(root, "bench.py"), "--gpus", "2",
           "--steps", "3", "--warmup", "1", "--workload", "opt-125m", "--replicas", "1",
           "--full", "--no-cpu-baseline", "--clock-warm-ms", "20", "--write-dir", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0
    assert line["config"]["elements"] == 125239296 and line["config"]["parallelism"].startswith("shard2")
    shapes = bench.shapes_of("opt-125m")
    owner = D.shard([int(torch.Size(s).numel()) for s in shapes], 2)
    want = 0
    for i, sh in enumerate(shapes):
        if owner[i] == 1:
            for (dims, dt) in bench.packed_out_shapes(sh, 4, 128).values():
                want += int(torch.Size(dims).numel()) * torch.empty((), dtype=dt).element_size()
    assert line["exchange"]["bytes_to_rank0"] == want
    assert line["roofline"]["read_dominant_ceiling"] > 0 and "cpu_baseline" not in line   # baseline: N=1 only
    # per-rank output leg: rank 0's packed shard written as chunk files, then removed
    assert line["write"]["bytes_rank0"] > 0 and line["write"]["s_max_over_ranks"] >= line["write"]["s_rank0"] > 0
    assert os.listdir(tmp_path) == []


def test_bench_defaults_north_star():
    """The default (driver-run) bench line is the north_star config: the Llama-3-70B tensor
    set, one copy LPT-sharded over the ranks (strong scaling), bf16, gs 128, 4-bit asym."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    a = bench.parse([])
    assert (a.workload, a.replica, a.dtype, a.group_size, a.bits, a.symmetric) == (
        "llama3-70b", False, "bf16", 128, 4, False)
    shapes = bench.shapes_of("llama3-70b")
    assert len(shapes) == 723 and sum(int(torch.Size(s).numel()) for s in shapes) == 70553706496
    with pytest.raises(SystemExit):
        bench.parse(["--replica", "--shard"])


def test_bench_cpu_baseline_extrapolates(monkeypatch):
    """cpu_baseline: C1 in full + a row sample of every distinct shape,
    extrapolated to the workload; cores = threads used, the node's CPU count beside it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    monkeypatch.setenv("OMP_NUM_THREADS", "2")
    cb = bench.cpu_baseline("opt-125m", 1.0)
    assert cb["kind"] == "port" and cb["cores"] == 2 and cb["node_cpus"] == os.cpu_count()
    assert cb["value"] > 0 and cb["c1_full"]["seconds"] > 0 and "EXTRAPOLATED" in cb["sample"]
    assert cb["shapes_sampled"] == len(bench.WORKLOADS["opt-125m"])


def test_bench_full_and_dump_flags():
    """--full (the legs beside the headline figure) is off by default; --dump-outputs takes a directory."""
    import bench
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d", "--steps", "7"])
    assert a.full is True and a.dump_outputs == "d" and a.steps == 7


def test_bench_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """dump_outputs: int32 words as float64, fp16 as float32; a tensor within its share of the
    byte budget is written whole, a larger one as a seeded sample at sorted positions, the same
    in every call."""
    import numpy as np
    import bench
    g = torch.Generator().manual_seed(3)
    big = torch.randint(-2 ** 31, 2 ** 31 - 1, (37, 101), generator=g, dtype=torch.int64).to(torch.int32)
    small = torch.tensor([[-2 ** 31, 2 ** 31 - 1, -1]], dtype=torch.int32)
    sc = [torch.randn(5, 7, generator=g).to(torch.float16), torch.randn(300, generator=g).to(torch.float16)]
    fields = {"qweight": [big, small], "scales": sc}
    # 2 fields: 1600 B each; qweight 200 float64 -> 100 per tensor, scales 400 float32 -> 200 per tensor
    monkeypatch.setattr(bench, "DUMP_BYTES", 3200)
    n = bench.dump_outputs(str(tmp_path / "a"), fields)
    assert n == {"qweight.npy": 103, "scales.npy": 235}
    qw, s = np.load(tmp_path / "a" / "qweight.npy"), np.load(tmp_path / "a" / "scales.npy")
    assert qw.dtype == np.float64 and s.dtype == np.float32
    assert qw.nbytes + s.nbytes <= 3200
    idx = torch.randint(big.numel(), (100,), generator=torch.Generator().manual_seed(bench.DUMP_SEED)).sort().values
    assert np.array_equal(qw[:100], big.reshape(-1)[idx].numpy().astype(np.float64))
    assert qw[100:].tolist() == [-2.0 ** 31, 2.0 ** 31 - 1, -1.0]
    assert np.array_equal(s[:35], sc[0].reshape(-1).float().numpy())
    idx = torch.randint(300, (200,), generator=torch.Generator().manual_seed(bench.DUMP_SEED + 1)).sort().values
    assert np.array_equal(s[35:], sc[1][idx].float().numpy())
    bench.dump_outputs(str(tmp_path / "b"), fields, prefix="rank1.")
    assert sorted(os.listdir(tmp_path / "b")) == ["rank1.qweight.npy", "rank1.scales.npy"]
    assert np.array_equal(np.load(tmp_path / "b" / "rank1.qweight.npy"), qw)


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
def test_bench_plain_and_full_run_gpu(tmp_path, monkeypatch, capsys, full):
    """One in-process bench run on the c1 workload.  A plain run times exactly --steps steps and
    prints the headline line with ms_per_step and neither the ceiling probe nor the CPU baseline;
    --full adds both.  --dump-outputs writes the last timed step's outputs: regenerated from the
    same seeds, they equal the oracle's bit for bit."""
    import numpy as np
    import bench
    from oracle import awq_oracle as orc
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path / "dump"
    argv = ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "c1", "--replicas", "1",
            "--clock-warm-ms", "20", "--dump-outputs", str(out)]
    if full:
        argv += ["--full", "--cpu-sample-seconds", "0.2"]
    monkeypatch.setattr(sys, "argv", argv)
    bench.main()
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert line["metric"] == bench.METRIC and line["unit"] == "GB/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["steps"] == 2 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1024 * 4096 * 2 / (line["ms_per_step"] / 1e3) / 1e9, rel=1e-2)
    assert 0 < line["roofline"]["frac"] < 1
    assert ("cpu_baseline" in line) == full and ("read_dominant_ceiling" in line["roofline"]) == full
    if full:
        assert line["cpu_baseline"]["value"] > 0 and line["roofline"]["read_dominant_ceiling"] > 0
    assert sorted(os.listdir(out)) == ["qweight.npy", "qzeros.npy", "scales.npy"]
    x = bench.make_set(bench.shapes_of("c1"), 0, torch.device("cuda", 0))["t0000"].cpu()
    ref = orc.quantize(x, bits=4, group_size=128, symmetric=False)
    want = {"qweight": orc.pack_rows(ref["tensor_q"], 4, 0), "qzeros": orc.pack_rows(ref["zero_points"], 4, 0),
            "scales": ref["scales"]}
    for f, w in want.items():
        got = np.load(out / f"{f}.npy")
        assert got.dtype == (np.float32 if f == "scales" else np.float64), f
        assert np.array_equal(got, w.reshape(-1).to(torch.float64).numpy()), f


def test_act_stats_file_and_flags(tmp_path):
    from awq_quantizer.main import load_act_stats, main, parse_args
    a = parse_args(["--model_id", "m", "--output_dir", "o", "--scale_method", "awq", "--act_stats", "s.st",
                    "--no_duo_scaling"])
    assert (a.scale_method, a.act_stats, a.no_duo_scaling) == ("awq", "s.st", True)
    p = str(tmp_path / "stats.safetensors")
    save_file({"a.weight.x_mean": torch.ones(4), "a.weight.x_sq": torch.full((4,), 2.0),
               "b.weight.x_mean": torch.ones(4)}, p)
    with pytest.raises(ValueError, match="x_sq"):
        load_act_stats(p)
    save_file({"a.weight.x_mean": torch.ones(4), "a.weight.x_sq": torch.full((4,), 2.0)}, p)
    st = load_act_stats(p)
    assert list(st) == ["a.weight"] and torch.equal(st["a.weight"][1], torch.full((4,), 2.0))
    d = _model_dir(tmp_path, _tensors())
    # statistics need scale_method awq; awq input scales cannot go into an AutoAWQ checkpoint unfolded
    assert main(["--model_id", d, "--output_dir", str(tmp_path / "o1"), "--act_stats", p, "--log_level",
                 "CRITICAL"]) == 1
    assert main(["--model_id", d, "--output_dir", str(tmp_path / "o2"), "--act_stats", p, "--scale_method", "awq",
                 "--output_format", "autoawq", "--log_level", "CRITICAL"]) == 1


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")
@pytest.mark.parametrize("fmt", ["packed", "reference"])
def test_main_act_stats_gpu(tmp_path, fmt):
    """--scale_method awq --act_stats: weights with statistics take the activation-aware
    search (equal to the oracle's, given the GPU's scale table) and carry input_scale; the
    others are RTN."""
    from awq_quantizer import _hip
    from awq_quantizer.main import main
    from oracle import awq_oracle as orc
    tensors = _tensors()
    d = _model_dir(tmp_path, tensors)
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(200, 768, generator=g) * (1 + 20 * (torch.rand(768, generator=g) < 0.05))).bfloat16()
    xm, xs = orc.act_stats(x)
    name = "model.layers.0.mlp.fc1.weight"
    p = str(tmp_path / "stats.safetensors")
    save_file({name + ".x_mean": xm, name + ".x_sq": xs}, p)
    out = tmp_path / "out"
    assert main(["--model_id", d, "--output_dir", str(out), "--scale_method", "awq", "--act_stats", p,
                 "--output_format", fmt, "--log_level", "ERROR"]) == 0
    meta = json.load(open(out / "metadata.json"))
    res = torch.load(str(out / f"model_chunk_{meta['tensor_to_chunk'][name]:04d}.pt"), weights_only=True)[name]
    w = tensors[name]
    dev = torch.device("cuda", 0)
    table = _hip.act_scale_table(xm.to(dev), _hip.weight_mean([w.to(dev)], 128), 20).cpu()
    ref = orc.awq_search([w], x_mean=xm, x_sq=xs, n_grid=20, symmetric=False, table=table)
    assert torch.equal(res["input_scale"], ref["input_scale"])
    rr = ref["results"][0]
    if fmt == "packed":
        assert torch.equal(res["qweight"], orc.pack_rows(rr["tensor_q"], 4, 0))
    else:
        assert torch.equal(res["tensor_q"], rr["tensor_q"])
    other = torch.load(str(out / f"model_chunk_{meta['tensor_to_chunk']['model.embed.weight']:04d}.pt"),
                       weights_only=True)["model.embed.weight"]
    assert "input_scale" not in other


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")
@pytest.mark.parametrize("packed", [True, False])
def test_native_stream_small_slots_split_rows(tmp_path, packed):
    """The native pipeline (include/awq_hip.h awq_stream_*) with 64 KiB staging slots: large
    tensors split by rows over many batches, slots reused many times, one-tensor and
    many-tensor batches, fp16 / fp32 / fp64 / bf16 items (ragged and per-tensor launches),
    padded rows (K % 128 != 0) and a K % 8 != 0 tensor — every result equals the oracle's."""
    import threading
    from oracle import awq_oracle as orc
    from awq_quantizer.main import quantize_stream_native
    from awq_quantizer.model_loading import load_model_from_path
    from awq_quantizer.quantization import AWQQuantizer
    g = torch.Generator().manual_seed(7)
    r = lambda *s, dt=torch.bfloat16: (torch.randn(*s, generator=g) * 0.02).to(dt)
    tensors = {"big": r(700, 512), "f16": r(96, 384, dt=torch.float16), "f32": r(40, 256, dt=torch.float32),
               "f64": r(33, 256, dt=torch.float64), "padded": r(50, 200), "odd": r(13, 203), "vec": r(4096),
               "t3": r(24, 3, 128)}
    for i in range(40):
        tensors[f"tiny{i}"] = r(128)
    d = _model_dir(tmp_path, tensors, files=3)
    loader = load_model_from_path(d, logger_level="ERROR")
    infos = loader.tensor_index()
    q = AWQQuantizer(bits=4, group_size=128, symmetric=False, device="cuda", logger_level="ERROR")
    out, done = {}, []
    quantize_stream_native(loader, infos, q, "cuda:0", 4, packed, out, threading.Lock(), None,
                           on_done=lambda n, res: done.append(n), slot_bytes=64 << 10)
    assert sorted(done) == sorted(tensors) == sorted(out)
    for name, x in tensors.items():
        ref = orc.quantize(x, bits=4, group_size=128, symmetric=False)
        res = out[name]
        rows = 1 if x.dim() <= 1 else x.shape[0]
        if packed:
            assert torch.equal(res["qweight"], orc.pack_rows(ref["tensor_q"].reshape(rows, -1), 4, 0)), name
            assert torch.equal(res["qzeros"], orc.pack_rows(ref["zero_points"], 4, 0)), name
            assert list(res["shape"]) == list(x.shape)
        else:
            assert torch.equal(res["tensor_q"], ref["tensor_q"]), name
            assert torch.equal(res["zero_points"], ref["zero_points"]), name
        assert torch.equal(res["scales"].view(torch.int16), ref["scales"].view(torch.int16)), name
    st = __import__("awq_quantizer.main", fromlist=["TIMINGS"]).TIMINGS["stream_cuda:0"]
    assert st["engine"] == "native" and st["batches"] > 10 and st["pieces"] > st["batches"]


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")
@pytest.mark.parametrize("fmt", ["packed", "reference"])
def test_cli_llama3_8b_shaped_multifile(tmp_path, fmt):
    """BASELINE config 4's tensor set (Llama-3-8B: 291 tensors, every shape) with rows cut to
    1/32 (K and the group structure kept), 4 safetensors files, through the CLI's native
    pipeline: every tensor equals the oracle."""
    import bench
    from oracle import awq_oracle as orc
    from awq_quantizer.main import main
    g = torch.Generator().manual_seed(8)
    tensors = {}
    for i, shape in enumerate(bench.shapes_of("llama3-8b")):
        shp = (max(1, shape[0] // 32),) + tuple(shape[1:]) if len(shape) == 2 else shape
        tensors[f"model.layers.{i // 9}.t{i}.weight"] = (torch.randn(*shp, generator=g) * 0.02).to(torch.bfloat16)
    d = _model_dir(tmp_path, tensors, files=4)
    out = tmp_path / "out"
    assert main(["--model_id", d, "--output_dir", str(out), "--log_level", "ERROR", "--output_format", fmt]) == 0
    meta = json.load(open(out / "metadata.json"))
    assert meta["num_tensors"] == len(tensors) == 291
    cache = {}
    for name, ci in meta["tensor_to_chunk"].items():
        if ci not in cache:
            cache = {ci: torch.load(str(out / f"model_chunk_{ci:04d}.pt"), weights_only=True)}
        res = cache[ci][name]
        x = tensors[name]
        ref = orc.quantize(x, bits=4, group_size=128, symmetric=False)
        if fmt == "packed":
            rows = 1 if x.dim() <= 1 else x.shape[0]
            assert torch.equal(res["qweight"], orc.pack_rows(ref["tensor_q"].reshape(rows, -1), 4, 0)), name
        else:
            assert torch.equal(res["tensor_q"], ref["tensor_q"]), name
            assert torch.equal(res["zero_points"], ref["zero_points"]), name
        assert torch.equal(res["scales"].view(torch.int16), ref["scales"].view(torch.int16)), name


def _ring_model():
    """~70 tensors of mixed sizes (row splits over 64 KiB slots, many-tensor batches)."""
    g = torch.Generator().manual_seed(11)
    r = lambda *s, dt=torch.bfloat16: (torch.randn(*s, generator=g) * 0.02).to(dt)
    t = {"big": r(700, 512), "f16": r(96, 384, dt=torch.float16), "f32": r(40, 256, dt=torch.float32),
         "padded": r(50, 200), "t3": r(24, 3, 128)}
    for i in range(30):
        t[f"mid{i}"] = r(8 + 4 * i, 256)
    for i in range(36):
        t[f"tiny{i}"] = r(128 + 64 * (i % 5))
    return t


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")
@pytest.mark.parametrize("fmt", ["packed", "reference"])
def test_native_stream_bounded_rings_wrap(tmp_path, monkeypatch, fmt):
    """ADVICE r3 (bounded output memory): 64 KiB staging slots and host / device output
    rings far smaller than the output, so both wrap — kernels wait on earlier D2H, copies
    wait on the chunk writer's releases — and every chunk file still holds the oracle's
    results."""
    from oracle import awq_oracle as orc
    from awq_quantizer import main as M
    tensors = _ring_model()
    d = _model_dir(tmp_path, tensors, files=3)
    for k, v in (("slot_bytes", 64 << 10), ("host_ring_bytes", 64 << 10), ("dev_ring_bytes", 64 << 10)):
        monkeypatch.setitem(M.STREAM_OPTS, k, v)
    out = tmp_path / "out"
    M.TIMINGS.clear()
    assert M.main(["--model_id", d, "--output_dir", str(out), "--log_level", "ERROR", "--chunk_size", "3",
                   "--output_format", fmt]) == 0
    (st,) = [v for k, v in M.TIMINGS.items() if k.startswith("stream_")]
    assert st["host_wraps"] and st["dev_wraps"], st
    total = sum(tensors[n].numel() for n in tensors) * (0.6 if fmt == "packed" else 4.2)
    assert st["host_ring_MB"] * (1 << 20) < total
    meta = json.load(open(out / "metadata.json"))
    assert meta["num_tensors"] == len(tensors)
    for name, ci in meta["tensor_to_chunk"].items():
        res = _load_chunk(out, ci, False)[name]
        x = tensors[name]
        ref = orc.quantize(x, bits=4, group_size=128, symmetric=False)
        if fmt == "packed":
            rows = 1 if x.dim() <= 1 else x.shape[0]
            assert torch.equal(res["qweight"], orc.pack_rows(ref["tensor_q"].reshape(rows, -1), 4, 0)), name
            assert torch.equal(res["qzeros"], orc.pack_rows(ref["zero_points"], 4, 0)), name
        else:
            assert torch.equal(res["tensor_q"], ref["tensor_q"]), name
            assert torch.equal(res["zero_points"], ref["zero_points"]), name
        assert torch.equal(res["scales"].view(torch.int16), ref["scales"].view(torch.int16)), name


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")
def test_native_stream_rings_wrap_with_failing_tensors(tmp_path, monkeypatch):
    """the host ring's sizing relies on ChunkWriter.predict_groups() placing chunks
    as the writer later does.  A float tensor the kernels do not take (float8: fails on the
    per-tensor path, before the pipeline's items), an int32 tensor and a sub-group tensor
    (both filtered by the CLI, main.py:241-253) next to the wrapping 64 KiB rings: every
    chunk, and metadata.json, still hold exactly the successful tensors' oracle results."""
    if not hasattr(torch, "float8_e4m3fn"):
        pytest.skip("no float8 in this torch")
    from oracle import awq_oracle as orc
    from awq_quantizer import main as M
    tensors = _ring_model()
    g = torch.Generator().manual_seed(12)
    extra = {"f8": (torch.randn(48, 256, generator=g) * 0.02).to(torch.float8_e4m3fn),
             "ints": torch.randint(-5, 5, (64, 128), generator=g, dtype=torch.int32),
             "small": (torch.randn(100, generator=g) * 0.02).to(torch.bfloat16)}
    d = _model_dir(tmp_path, {**tensors, **extra}, files=3)
    for k, v in (("slot_bytes", 64 << 10), ("host_ring_bytes", 64 << 10), ("dev_ring_bytes", 64 << 10)):
        monkeypatch.setitem(M.STREAM_OPTS, k, v)
    out = tmp_path / "out"
    M.TIMINGS.clear()
    assert M.main(["--model_id", d, "--output_dir", str(out), "--log_level", "ERROR", "--chunk_size", "3",
                   "--output_format", "packed"]) == 0
    (st,) = [v for k, v in M.TIMINGS.items() if k.startswith("stream_")]
    assert st["host_wraps"] and st["dev_wraps"], st
    meta = json.load(open(out / "metadata.json"))
    assert meta["num_tensors"] == len(tensors) and sorted(meta["tensor_to_chunk"]) == sorted(tensors)
    counts = {}
    for name, ci in meta["tensor_to_chunk"].items():
        counts[ci] = counts.get(ci, 0) + 1
        res = _load_chunk(out, ci, False)[name]
        x = tensors[name]
        ref = orc.quantize(x, bits=4, group_size=128, symmetric=False)
        rows = 1 if x.dim() <= 1 else x.shape[0]
        assert torch.equal(res["qweight"], orc.pack_rows(ref["tensor_q"].reshape(rows, -1), 4, 0)), name
        assert torch.equal(res["scales"].view(torch.int16), ref["scales"].view(torch.int16)), name
    assert sorted(counts.values())[1:] == [3] * (len(counts) - 1)      # full chunks but the last


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")
def test_native_stream_failed_chunk_write_does_not_hang(tmp_path, monkeypatch):
    """a chunk write that raises (ENOSPC, I/O error) while the host
    ring wraps used to leave the pipeline waiting forever for a release.  Now the failed
    chunk's range is released, the producer stops at its next result, and main() returns
    non-zero — within seconds."""
    import threading as th
    from awq_quantizer import main as M, output as O
    d = _model_dir(tmp_path, _ring_model(), files=3)
    for k, v in (("slot_bytes", 64 << 10), ("host_ring_bytes", 64 << 10), ("dev_ring_bytes", 64 << 10)):
        monkeypatch.setitem(M.STREAM_OPTS, k, v)
    real = O._write_chunk
    calls = []

    def failing(chunk, output_dir, c, *a, **kw):
        calls.append(c)
        if c == 2:
            raise OSError(28, "No space left on device (injected)")
        return real(chunk, output_dir, c, *a, **kw)

    monkeypatch.setattr(O, "_write_chunk", failing)
    rc = []
    t = th.Thread(target=lambda: rc.append(M.main(["--model_id", d, "--output_dir", str(tmp_path / "out"),
                                                  "--log_level", "CRITICAL", "--chunk_size", "3",
                                                  "--output_format", "packed"])), daemon=True)
    t.start()
    t.join(90)
    assert not t.is_alive(), "main() hung after a failed chunk write"
    assert rc == [1] and 2 in calls


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")
def test_cli_search_native_engine_equals_python_engine(tmp_path):
    """--scale_method search through the default (native) engine runs the clip
    search (awq_quantize_search_ex per piece), with the Python engine's exact bits — and
    not plain RTN."""
    from awq_quantizer.main import main
    tensors = _tensors()
    d = _model_dir(tmp_path, tensors, files=2)
    got = {}
    for engine in ("native", "python"):
        out = tmp_path / engine
        assert main(["--model_id", d, "--output_dir", str(out), "--log_level", "ERROR", "--scale_method", "search",
                     "--output_format", "packed", "--stream_engine", engine]) == 0
        meta = json.load(open(out / "metadata.json"))
        got[engine] = {n: _load_chunk(out, c, False)[n] for n, c in meta["tensor_to_chunk"].items()}
    rtn = tmp_path / "rtn"
    assert main(["--model_id", d, "--output_dir", str(rtn), "--log_level", "ERROR", "--output_format", "packed"]) == 0
    meta = json.load(open(rtn / "metadata.json"))
    plain = {n: _load_chunk(rtn, c, False)[n] for n, c in meta["tensor_to_chunk"].items()}
    assert sorted(got["native"]) == sorted(got["python"]) == sorted(plain)
    differs = False
    for n in plain:
        for f in ("qweight", "qzeros", "scales"):
            a, b = got["native"][n][f], got["python"][n][f]
            assert torch.equal(a.view(torch.int16) if f == "scales" else a,
                               b.view(torch.int16) if f == "scales" else b), (n, f)
        differs |= not torch.equal(got["native"][n]["scales"].view(torch.int16), plain[n]["scales"].view(torch.int16))
    assert differs
