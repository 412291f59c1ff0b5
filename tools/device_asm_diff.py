#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two checkouts, kernel by kernel (CPU only: it cross-compiles, nothing runs).

    tools/device_asm_diff.py PARENT BRANCH [--files a.hip b.hip ...] [--rename OLD=NEW ...] [--jobs N] [--show N] [--keep DIR]

Every listed translation unit (default: SRCS of BRANCH's csrc/Makefile) of both checkouts is compiled with the Makefile's device
flags (`-O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S`, the file's EXTRA_FLAGS, a fixed `-cuid`).  The assembly
is split at every `.globl` (what follows the last function, the metadata, is one more piece); comment, `.ident` and `.file` lines go, mangled names and the function numbers inside local labels
become placeholders.  Kernels are matched by position, or by name where `--rename OLD=NEW` gives a substring of the parent's
mangled name and what stands in its place in the branch's.  Per kernel it prints equal / DIFFERENT with code length, VGPRs, AGPRs
and scratch of both sides; the exit status is non-zero on any difference.  It compares two text files and inspects nothing in them.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BASE_FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-cuid=device_asm_diff"]
CSRC = os.path.join("rusty_compression_amd", "csrc")
FIGURES = (("len", r"; codeLenInByte = (\d+)"), ("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"),
           ("scratch", r"; ScratchSize: (\d+)"))
MANGLED = re.compile(r"_Z[A-Za-z0-9_$.]+")
LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+")


def makefile_lists(root):
    """SRCS and the per-file EXTRA_FLAGS of csrc/Makefile."""
    text = open(os.path.join(root, CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", text, re.M).group(1).split()
    extra = {m.group(1) + ".hip": m.group(2).split()
             for m in re.finditer(r"^\$\(OBJDIR\)/(\w+)\.o: EXTRA_FLAGS := (.*)$", text, re.M)}
    return srcs, extra


def compile_asm(root, src, extra, out):
    cmd = [HIPCC] + BASE_FLAGS + extra + [os.path.join(root, CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stderr))
    return out


def split_kernels(path):
    """[(mangled name, figures, normalised lines)] in file order; what follows the last function is the entry '<tail>'."""
    segs = [["<head>", []]]
    for line in open(path):
        m = re.match(r"\s*\.globl\s+(\S+)", line)
        if m:
            segs.append([m.group(1), []])
        elif line.startswith("\t.amdgpu_metadata"):
            segs.append(["<tail>", []])
        segs[-1][1].append(line)
    out = []
    for name, lines in segs:
        raw = "".join(lines)
        fig = {k: (int(m.group(1)) if (m := re.search(p, raw)) else None) for k, p in FIGURES}
        norm = []
        for line in lines:
            s = line.strip()
            if not s or s.startswith(";") or s.startswith(".ident") or s.startswith(".file"):
                continue
            if not s.startswith((".asci", ".string")):
                s = re.sub(r"\s+;.*$", "", s)
            norm.append(LOCAL.sub(r".L\1#", MANGLED.sub("@", s)))
        out.append((name, fig, norm))
    return out


def fig_text(f):
    return "len %s vgpr %s agpr %s scratch %s" % tuple(f[k] for k, _ in FIGURES)


def compare(src, a, b, renames, show=0):
    """Prints one line per kernel of b; returns the number of differences."""
    ka, kb = split_kernels(a), split_kernels(b)
    bad = 0
    if renames:
        by_name = {n: (n, f, l) for n, f, l in kb}
        pairs = []
        for n, f, l in ka:
            want = n
            for old, new in renames:
                want = want.replace(old, new)
            pairs.append(((n, f, l), by_name.get(want)))
    else:
        pairs = [(x, kb[i] if i < len(kb) else None) for i, x in enumerate(ka)]
    extra_b = max(0, len(kb) - len(ka))
    for x, y in pairs:
        if y is None:
            print("%s: MISSING in branch  %s" % (src, x[0]))
            bad += 1
            continue
        same = x[2] == y[2]
        bad += not same
        if x[1]["len"] is None and y[1]["len"] is None:  # not a function: the head, a variable, the metadata
            if not same:
                print("%s: DIFFERENT  %s" % (src, x[0]))
            continue
        print("%s: %s  %s | %s  %s%s" % (src, "equal" if same else "DIFFERENT", fig_text(x[1]), fig_text(y[1]), y[0],
                                       "" if x[0] == y[0] else "  (was %s)" % x[0]))
        if show and not same:
            print("\n".join(list(difflib.unified_diff(x[2], y[2], "parent", "branch", lineterm="", n=1))[:show]))
    if extra_b:
        print("%s: %d more functions in branch than in parent" % (src, extra_b))
        bad += extra_b
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--files", nargs="+", help="translation units to compare (default: SRCS of the branch's Makefile)")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="match kernels by name after this replacement")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N lines of each different kernel's diff")
    ap.add_argument("--keep", help="directory that keeps the .s files (default: a temporary one)")
    args = ap.parse_args()
    srcs, extra_b = makefile_lists(args.branch)
    extra_a = makefile_lists(args.parent)[1]
    srcs = args.files or srcs
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    tmp = None
    if args.keep:
        os.makedirs(args.keep, exist_ok=True)
        work = args.keep
    else:
        tmp = tempfile.TemporaryDirectory()
        work = tmp.name
    bad = 0
    with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        jobs = {}
        for src in srcs:
            stem = src[:-len(".hip")]
            jobs[src] = [pool.submit(compile_asm, root, src, extra.get(src, []), os.path.join(work, "%s.%s.s" % (stem, side)))
                         for side, root, extra in (("parent", args.parent, extra_a), ("branch", args.branch, extra_b))]
        for src in srcs:
            bad += compare(src, jobs[src][0].result(), jobs[src][1].result(), renames, args.show)
    print("%d of %d translation units compared, %d differences" % (len(srcs), len(srcs), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
