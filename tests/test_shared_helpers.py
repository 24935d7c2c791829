"""One definition per shared helper in awq-converter_amd/csrc (CPU only, a text search).

The device primitives every kernel file needs (the DPP step, the group and wave reductions, the
verified reciprocals and roundings, the value barrier, the Markstein quotient, the buffer
descriptor) live in awq_lanes.h / awq_quant.h, the host helpers of the entry points in
awq_capi.hip (declared in awq_internal.h).  A private copy in a kernel file is how four
spellings of one summation tree came about: a fix to one copy misses the others, and a selftest
only proves the copy it compiles.  This test fails when a name of the list below is defined at
namespace scope in more than one file, or not at all.  A second search keeps each kernel at one
path: preprocessor conditionals may only test the AWQ_* names of CONDITIONAL_MACROS.
"""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "awq-converter_amd", "csrc")

# helper -> the file that owns it
HELPERS = {
    # awq_lanes.h: the DPP step, the row / half swaps, group and whole-wave reductions
    "dpp_mov": "awq_lanes.h", "dpp_add": "awq_lanes.h", "swap16": "awq_lanes.h", "swap32": "awq_lanes.h",
    "grp_sum": "awq_lanes.h", "grp_max": "awq_lanes.h", "grp_or": "awq_lanes.h",
    "grp_minmax": "awq_lanes.h", "grp_minmax_nn": "awq_lanes.h",
    "wave_sum": "awq_lanes.h", "wave_min": "awq_lanes.h", "wave_max": "awq_lanes.h",
    "wave_max_up": "awq_lanes.h", "wave_or": "awq_lanes.h",
    # awq_quant.h: per-dtype arithmetic
    "recip_bf16": "awq_quant.h", "recip_f16": "awq_quant.h", "rn_bf16": "awq_quant.h",
    "opaque": "awq_quant.h", "mquot": "awq_quant.h", "mquot_h": "awq_quant.h", "mprod_h": "awq_quant.h",
    "rsrc": "awq_quant.h",
    # awq_capi.hip: host helpers (declared in awq_internal.h)
    "aligned": "awq_capi.hip", "fail": "awq_capi.hip", "set_error": "awq_capi.hip", "hip_status": "awq_capi.hip",
}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def definitions(text, name):
    """Namespace-scope function definitions of `name`: a line that starts in column 0 with a
    return type, then name(parameters) and an opening brace (a declaration ends in ';')."""
    pat = re.compile(r"^[A-Za-z_][\w \t\*&:<>,]*?[ \t\*&]%s[ \t]*\([^;{}]*?\)[ \t\n]*\{" % re.escape(name), re.M)
    return pat.findall(_strip_comments(text))


def prototypes(text, name):
    pat = re.compile(r"^[A-Za-z_][\w \t\*&:<>,]*?[ \t\*&]%s[ \t]*\([^;{}]*?\)[^;{}]*;" % re.escape(name), re.M)
    return pat.findall(_strip_comments(text))


def _sources():
    out = {}
    for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        with open(p, errors="replace") as f:
            out[os.path.basename(p)] = f.read()
    return out


def test_search_sees_definitions_and_skips_other_uses():
    text = ("namespace awq {\n"
            "int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));\n"
            "template <int CTRL>\n__device__ __forceinline__ float dpp_mov(float v) {\n    return v;\n}\n"
            "__device__ __forceinline__ float mquot(float a, float s,\n                                 float rs) {\n"
            "    return fail(1, \"x\");\n}\n"
            "struct P {\n    void fail(int code) { (void)code; }\n};\n"
            "// int fail(int code) { a comment }\n"
            "int fail(int code, const char* fmt, ...) {\n    return code;\n}\n}\n")
    assert len(definitions(text, "fail")) == 1
    assert len(prototypes(text, "fail")) == 1
    assert len(definitions(text, "dpp_mov")) == 1
    assert len(definitions(text, "mquot")) == 1
    assert definitions(text, "quot") == []


@pytest.mark.parametrize("name", sorted(HELPERS))
def test_helper_is_defined_in_one_file(name):
    found = {f: len(definitions(t, name)) for f, t in _sources().items()}
    found = {f: n for f, n in found.items() if n}
    assert list(found) == [HELPERS[name]], f"{name} is defined in {found}, expected only {HELPERS[name]}"


# AWQ_* names a preprocessor conditional in csrc may test.  A compile-time A/B switch whose
# default is the adopted path leaves a branch nobody builds in the middle of a kernel: once the
# measurement is settled the switch goes, so a new one has to be added here on purpose.
CONDITIONAL_MACROS = {
    "AWQ_DIAG_H", "AWQ_LANES_H", "AWQ_QUANT_H",                     # header guards
    "AWQ_DIAG", "AWQ_TRACE",                                        # the tool builds
    # numeric tunables
    "AWQ_WPB", "AWQ_SEARCH_MIN_WAVES", "AWQ_MIN_WAVES", "AWQ_MIN_WAVES_WIDE", "AWQ_LOAD_AUX", "AWQ_STORE_AUX",
    "AWQ_SMALL_AUX", "AWQ_EXPORT_NT_MIN", "AWQ_RG_UNROLL",
}


def test_preprocessor_conditionals_test_only_listed_macros():
    found = {}
    for f, text in _sources().items():
        for line in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b[^\n]*", text, re.M):
            for name in re.findall(r"\bAWQ_\w+", line):
                found.setdefault(name, set()).add(f)
    assert {"AWQ_DIAG", "AWQ_TRACE"} <= set(found), "the search no longer sees the conditionals"
    extra = {n: sorted(fs) for n, fs in found.items() if n not in CONDITIONAL_MACROS}
    assert not extra, f"preprocessor conditionals test macros that are not on the allow-list: {extra}"


def test_host_helpers_are_declared_once():
    # no hand-written prototype next to the one in awq_internal.h
    for name in ("set_error", "fail", "hip_status", "aligned"):
        found = [f for f, t in _sources().items() if prototypes(t, name)]
        assert found == ["awq_internal.h"], f"{name} is declared in {found}"
