"""The CLI's flag rules (awq_quantizer/options.py check_flags / check_args) as a table: argv ->
the message main() logs before it exits 1, or None for a run that may start.  No model, no
device.  Also: the names main.py re-exports are the objects of the modules that own them."""
import pytest

BASE = ["--model_id", "m", "--output_dir", "o"]
AWQ = ["--scale_method", "awq"]
STATS = AWQ + ["--act_stats", "s.safetensors"]
CALIB = AWQ + ["--calib_ids", "ids.safetensors"]
FOLD = STATS + ["--output_format", "autoawq", "--fold_scales"]

E_BOTH = "--calib_ids and --act_stats are mutually exclusive: the statistics come from one of them"
E_FOLD_NEEDS = "--fold_scales needs --scale_method awq, --act_stats and --output_format autoawq"
E_BITS = "--output_format autoawq writes 4-bit checkpoints (AutoAWQ GEMM layout)"
E_FOLD_TYPE = "--fold_scales knows the block layout of model types llama, mistral, qwen2; config.json says {!r}"
E_FOLD_WORLD = "--fold_scales runs in one process (sharding by block under torchrun is not implemented)"
E_FOLD_DEVS = "--fold_scales runs on one GPU, not on {} (--multi_gpu / --device all): name one with --device"
E_CLIP_NEEDS = "--act_clip needs --scale_method awq and --act_stats"
E_CLIP_PACKED = "--act_clip writes packed results only: use --output_format packed"
E_CLIP_RANGE = "--act_clip needs --clip_grid >= 1 and --clip_max_shrink in [0, 1]"
E_STATS_AWQ = "{} needs --scale_method awq"
E_STATS_AUTOAWQ = ("--act_stats with --output_format autoawq: the searched input scales must be folded "
                   "into the ops producing each input first; use --output_format packed or reference "
                   "(results carry 'input_scale'), or add --fold_scales")

# (label, argv after BASE, world, n_devices, model_type, expected)
CASES = [
    # one full argv per valid mode
    ("reference", [], 1, 1, None, None),
    ("packed", ["--output_format", "packed"], 1, 1, None, None),
    ("packed, 8 bits, two devices", ["--output_format", "packed", "--bits", "8"], 1, 2, None, None),
    ("packed under torchrun", ["--output_format", "packed"], 8, 1, None, None),
    ("autoawq", ["--output_format", "autoawq"], 1, 1, "opt", None),
    ("autoawq under torchrun", ["--output_format", "autoawq"], 2, 1, "llama", None),
    ("autoawq with --fold_scales", FOLD, 1, 1, "llama", None),
    ("autoawq with --fold_scales, calibrated, clipped",
     CALIB + ["--output_format", "autoawq", "--fold_scales", "--act_clip"], 1, 1, "qwen2", None),
    ("--act_clip packed", STATS + ["--output_format", "packed", "--act_clip"], 1, 1, None, None),
    ("--act_clip packed at the ends of its ranges",
     STATS + ["--output_format", "packed", "--act_clip", "--clip_grid", "1", "--clip_max_shrink", "1.0"], 1, 1, None, None),
    ("statistics to the reference format", STATS, 1, 1, None, None),
    ("awq without statistics: a warning, not an error", AWQ, 1, 1, None, None),
    # every rule on its own
    ("both sources of statistics", STATS + ["--calib_ids", "i.npy"], 1, 1, None, E_BOTH),
    ("fold without awq", ["--act_stats", "s", "--output_format", "autoawq", "--fold_scales"], 1, 1, "llama", E_FOLD_NEEDS),
    ("fold without statistics", AWQ + ["--output_format", "autoawq", "--fold_scales"], 1, 1, "llama", E_FOLD_NEEDS),
    ("fold without autoawq", STATS + ["--output_format", "packed", "--fold_scales"], 1, 1, "llama", E_FOLD_NEEDS),
    ("autoawq at 8 bits", ["--output_format", "autoawq", "--bits", "8"], 1, 1, "llama", E_BITS),
    ("fold, unknown model type", FOLD, 1, 1, "opt", E_FOLD_TYPE.format("opt")),
    ("fold, no config.json", FOLD, 1, 1, None, E_FOLD_TYPE.format(None)),
    ("fold under torchrun", FOLD, 2, 1, "llama", E_FOLD_WORLD),
    ("fold on several devices", FOLD, 1, 8, "mistral", E_FOLD_DEVS.format(8)),
    ("clip without awq", ["--act_stats", "s", "--output_format", "packed", "--act_clip"], 1, 1, None, E_CLIP_NEEDS),
    ("clip without statistics", AWQ + ["--output_format", "packed", "--act_clip"], 1, 1, None, E_CLIP_NEEDS),
    ("clip to the reference format", STATS + ["--act_clip"], 1, 1, None, E_CLIP_PACKED),
    ("clip grid 0", STATS + ["--output_format", "packed", "--act_clip", "--clip_grid", "0"], 1, 1, None, E_CLIP_RANGE),
    ("clip shrink above 1", STATS + ["--output_format", "packed", "--act_clip", "--clip_max_shrink", "1.5"], 1, 1, None,
     E_CLIP_RANGE),
    ("clip shrink below 0", STATS + ["--output_format", "packed", "--act_clip", "--clip_max_shrink", "-0.1"], 1, 1, None,
     E_CLIP_RANGE),
    ("--act_stats without awq", ["--act_stats", "s"], 1, 1, None, E_STATS_AWQ.format("--act_stats")),
    ("--calib_ids without awq", ["--scale_method", "search", "--calib_ids", "i"], 1, 1, None,
     E_STATS_AWQ.format("--calib_ids")),
    ("statistics to autoawq, unfolded", STATS + ["--output_format", "autoawq"], 1, 1, "llama", E_STATS_AUTOAWQ),
    ("calibrated statistics to autoawq, unfolded", CALIB + ["--output_format", "autoawq"], 1, 1, "llama", E_STATS_AUTOAWQ),
    # several rules at once: the order main() has always reported them in
    ("both sources beat fold's prerequisites",
     ["--act_stats", "s", "--calib_ids", "i", "--output_format", "packed", "--fold_scales"], 1, 1, None, E_BOTH),
    ("fold's prerequisites beat 8-bit autoawq",
     ["--act_stats", "s", "--output_format", "autoawq", "--bits", "8", "--fold_scales"], 1, 1, "opt", E_FOLD_NEEDS),
    ("8-bit autoawq beats fold's model type", FOLD + ["--bits", "8"], 2, 4, "opt", E_BITS),
    ("fold: model type beats torchrun beats devices", FOLD, 2, 4, "opt", E_FOLD_TYPE.format("opt")),
    ("fold: torchrun beats devices", FOLD, 2, 4, "llama", E_FOLD_WORLD),
    ("fold's devices beat the clip range", FOLD + ["--act_clip", "--clip_grid", "0"], 1, 2, "llama", E_FOLD_DEVS.format(2)),
    ("clip's prerequisites beat its format", ["--act_clip"], 1, 1, None, E_CLIP_NEEDS),
    ("clip's format beats its range", STATS + ["--act_clip", "--clip_grid", "0"], 1, 1, None, E_CLIP_PACKED),
    ("clip's format beats unfolded autoawq", STATS + ["--output_format", "autoawq", "--act_clip"], 1, 1, "llama",
     E_CLIP_PACKED),
    ("clip's prerequisites beat statistics without awq",
     ["--act_stats", "s", "--output_format", "packed", "--act_clip"], 1, 1, None, E_CLIP_NEEDS),
    ("8-bit autoawq beats unfolded statistics", STATS + ["--output_format", "autoawq", "--bits", "8"], 1, 1, "llama",
     E_BITS),
]


@pytest.mark.parametrize("label,argv,world,n_devices,model_type,expected", CASES, ids=[c[0] for c in CASES])
def test_check_args(label, argv, world, n_devices, model_type, expected):
    from awq_quantizer.options import check_args, parse_args
    assert check_args(parse_args(BASE + argv), world, n_devices, model_type) == expected


def test_check_flags_is_the_part_main_applies_before_the_model_is_opened():
    """check_flags: exactly the first two rules, whatever else is wrong with the flags."""
    from awq_quantizer.options import check_flags, parse_args
    for label, argv, *_, expected in CASES:
        want = expected if expected in (E_BOTH, E_FOLD_NEEDS) else None
        assert check_flags(parse_args(BASE + argv)) == want, label


def test_derived_settings():
    from awq_quantizer.options import act_clip_of, has_stats, parse_args
    a = parse_args(BASE + STATS + ["--act_clip", "--clip_grid", "7", "--clip_max_shrink", "0.25"])
    assert has_stats(a) and act_clip_of(a) == {"clip_grid": 7, "clip_max_shrink": 0.25}
    assert has_stats(parse_args(BASE + CALIB))
    a = parse_args(BASE + ["--clip_grid", "7"])
    assert not has_stats(a) and act_clip_of(a) is None


def test_main_reexports_the_owning_modules_objects():
    """bench.py and the measurement scripts reach these through awq_quantizer.main; TIMINGS and
    STREAM_OPTS are mutated in place there, so each must be the one dict the pipeline uses."""
    from awq_quantizer import main, options, output, pipeline
    from awq_quantizer.main import ChunkWriter, _rank_stem
    assert main.TIMINGS is pipeline.TIMINGS and main.STREAM_OPTS is pipeline.STREAM_OPTS
    assert output.TIMINGS is pipeline.TIMINGS and output.STREAM_OPTS is pipeline.STREAM_OPTS
    assert ChunkWriter is output.ChunkWriter and _rank_stem is output._rank_stem
    assert main.quantize_stream_native is pipeline.quantize_stream_native
    assert main.parse_args is options.parse_args and main.save_model_in_chunks is output.save_model_in_chunks
    assert main.run_metrics is output.run_metrics
