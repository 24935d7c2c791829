#!/usr/bin/env python3
"""Compare the generated gfx950 assembly of every csrc/*.hip source against another revision.

    scripts/isa_diff.py REV [--keep DIR] [--only awq_fast.hip ...] [-j N]

For every .hip file of the csrc Makefile's SRCS, compiles the file as it stands in the working
tree and as it stood at REV (exported with `git archive` into a scratch directory) with the
Makefile's HIPFLAGS plus `--cuda-device-only -S`, once plain and once with -DAWQ_DIAG, and
compares the two assembly texts after dropping comment lines, .file / .ident / .loc lines and
lines that name the per-source hash symbol __hip_cuid_*, and after taking the function's ordinal
out of local labels (removing a kernel renumbers the labels of every later one; its own lines
still show as removed).  Exit status 0 = every file identical:
the bar for a refactor that must not change a kernel.  Needs only hipcc, no GPU.

--keep DIR keeps the assembly (DIR/REV-ish/..., DIR/head/...) and reuses REV's if it is already
there, so an edit-compile-compare loop only pays for the head.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("awq-converter_amd", "csrc")


def make_var(text, name):
    m = re.search(r"^%s\s*[:?]?=\s*((?:.*\\\n)*.*)$" % re.escape(name), text, re.M)
    if not m:
        raise SystemExit("isa_diff: no %s in the csrc Makefile" % name)
    return m.group(1).replace("\\\n", " ").split()


def makefile_vars(tree):
    with open(os.path.join(tree, CSRC, "Makefile")) as f:
        text = f.read()
    arch = make_var(text, "ARCH")[0]
    flags = [w.replace("$(ARCH)", arch) for w in make_var(text, "HIPFLAGS")]
    hipcc = os.environ.get("HIPCC") or make_var(text, "HIPCC")[0]
    return hipcc, flags, make_var(text, "SRCS")


def normalize(path):
    out = []
    with open(path, errors="replace") as f:
        for line in f:
            s = line.strip()
            if not s or s.startswith(";") or s.startswith("//") or "__hip_cuid_" in s:
                continue
            if re.match(r"\.(file|ident|loc)\b", s):
                continue
            # local labels carry the function's ordinal in the file (.LBB<f>_<block>, .Lfunc_end<f>):
            # removing a kernel renumbers every later one, no code changes (a label's loop comment,
            # padded to a column, goes too)
            if s.startswith(".LBB"):
                line = line.split(";")[0]
            line = re.sub(r"\b(L?BB)\d+_(\d+)", r"\1_\2", line)
            line = re.sub(r"(\.Lfunc_(?:begin|end))\d+", r"\1", line)
            out.append(line.rstrip())
    return out


def compile_one(job):
    hipcc, flags, tree, src, diag, out = job
    if os.path.exists(out):
        return out, ""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [hipcc] + flags + (["-DAWQ_DIAG"] if diag else []) + ["--cuda-device-only", "-S", src, "-o", out + ".tmp"]
    p = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        return None, "%s (%s%s):\n%s" % (src, tree, ", diag" if diag else "", p.stdout)
    os.replace(out + ".tmp", out)
    return out, ""


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev")
    ap.add_argument("--keep", metavar="DIR")
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--show", type=int, default=20, help="differing lines printed per file")
    a = ap.parse_args()

    sha = subprocess.check_output(["git", "rev-parse", "--short=12", a.rev + "^{commit}"], cwd=ROOT, text=True).strip()
    tmp = None
    if a.keep:
        work = os.path.abspath(a.keep)
        os.makedirs(work, exist_ok=True)
    else:
        tmp = tempfile.TemporaryDirectory(prefix="isa_diff_")
        work = tmp.name
    base_tree = os.path.join(work, sha, "tree")
    if not os.path.isdir(base_tree):
        os.makedirs(base_tree)
        ar = subprocess.Popen(["git", "archive", sha, CSRC, "include"], cwd=ROOT, stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", base_tree], stdin=ar.stdout)
        if ar.wait() != 0:
            raise SystemExit("isa_diff: git archive failed")

    hipcc, flags, srcs = makefile_vars(ROOT)
    _, base_flags, base_srcs = makefile_vars(base_tree)
    if a.only is not None:
        srcs = [s for s in srcs if s in a.only]
    jobs, pairs = [], []
    for src in srcs:
        if src not in base_srcs:
            print("NEW   %s (not in %s)" % (src, sha))
            continue
        for diag in (False, True):
            name = src[:-4] + (".diag.s" if diag else ".s")
            b = os.path.join(work, sha, "asm", name)
            h = os.path.join(work, "head", name)
            if os.path.exists(h):
                os.remove(h)
            jobs.append((hipcc, base_flags, base_tree, src, diag, b))
            jobs.append((hipcc, flags, ROOT, src, diag, h))
            pairs.append((src, diag, b, h))
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, a.j)) as ex:
        failed = [err for out, err in ex.map(compile_one, jobs) if out is None]
    if failed:
        sys.stderr.write("\n".join(failed))
        return 2

    bad = 0
    for src, diag, b, h in pairs:
        tag = "%s%s" % (src, " -DAWQ_DIAG" if diag else "")
        x, y = normalize(b), normalize(h)
        if x == y:
            print("SAME  %-32s %d lines" % (tag, len(y)))
            continue
        bad += 1
        delta = [d for d in difflib.unified_diff(x, y, sha, "head", n=0, lineterm="")
                 if d[:1] in "+-" and d[:3] not in ("+++", "---")]
        print("DIFF  %-32s %d differing lines" % (tag, len(delta)))
        for d in delta[:a.show]:
            print("      " + d)
    print("%d of %d assembly texts differ from %s" % (bad, len(pairs), sha))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
