#!/usr/bin/env python3
"""Did a change move any kernel?  Compiles two sets of .hip files to gfx950 assembly with the project's flags (host only, no GPU) and
compares, for every __global__ symbol, what the compiler emitted:

  text        the lines between the kernel's label and its .Lfunc_end (comments dropped, the function index in local labels normalised:
              it counts the functions of the translation unit, so it changes when a kernel moves to another file)
  descriptor  the kernel's .amdhsa_kernel block (registers, LDS, scratch, kernarg size, float mode, ...)
  metadata    the kernel's entry under amdhsa.kernels in .amdgpu_metadata (arguments, register counts, spills, workgroup size, ...)

It is a plain diff: it looks for no particular instruction.  One line per kernel; exit status 1 on any difference or when a kernel exists
on one side only.

  # the working tree's extractor files against the single file they were cut from
  tools/kernel_text_diff.py --a-rev HEAD --a orbx_extract.hip --b orbx_extract.hip orbx_pyramid.hip orbx_fast.hip orbx_tree.hip orbx_desc.hip
  # every file, parent commit against working tree, diagnostic build
  tools/kernel_text_diff.py --a-rev HEAD~1 --flags=-DORBX_DIAG

A name without a directory is a file of orb-slam2_amd/csrc; --a-rev / --b-rev take that directory (headers included) from a commit
instead of the working tree.  Without --a / --b a side is every .hip file of its directory."""
import argparse
import difflib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIPCC_FLAGS  # noqa: E402

CSRC = "orb-slam2_amd/csrc"
LINK_ONLY = {"-shared"}


def assembly(path, extra, tmp):
    out = os.path.join(tmp, "k%d.s" % len(os.listdir(tmp)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + [f for f in HIPCC_FLAGS if f not in LINK_ONLY] + extra + ["--cuda-device-only", "-S", "-o", out, path])
    return open(out).read()


def normalise(line):
    line = re.sub(r"\s+;.*$", "", line.rstrip())
    line = re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+", r".L\1N", line)
    return re.sub(r"\s+", " ", line.strip())


def kernels(asm):
    """{symbol: {"text": [...], "descriptor": [...], "metadata": [...]}} of one assembly file"""
    lines = asm.splitlines()
    res = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        name = m.group(1)
        j = next(k for k in range(i, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
        top = next(n for n, x in enumerate(lines) if x.startswith(name + ":"))
        end = next(n for n in range(top, len(lines)) if lines[n].startswith(".Lfunc_end"))
        body = lines[top + 1:end] if not top < i < end else lines[top + 1:i] + lines[j + 1:end]    # (the descriptor block sits inside the function's range)
        # the descriptor's register counts are expressions over symbols the compiler sets behind the function: ".set <kernel>.num_vgpr, 48"
        sets = [x for x in lines if re.match(r"\s*\.set\s+" + re.escape(name) + r"\.", x)]
        res[name] = {"text": [t for t in (normalise(x) for x in body if not x.lstrip().startswith(";")) if t],
                     "descriptor": [normalise(x) for x in lines[i + 1:j] + sets], "metadata": None}
    # metadata: the entries of the amdhsa.kernels list start with "  - " at the list's own indentation (their .args items sit deeper)
    md = asm.split(".amdgpu_metadata", 1)[1].split(".end_amdgpu_metadata", 1)[0].splitlines() if res else []
    starts = [n for n, l in enumerate(md) if l.startswith("  - ") and n > md.index("amdhsa.kernels:")]
    for a, b in zip(starts, starts[1:] + [len(md)]):
        entry = list(md[a:b])
        while entry and not entry[-1].startswith("  "):      # the keys behind the list (amdhsa.target, amdhsa.version)
            entry.pop()
        entry = [x for x in entry if x.startswith("  ")]
        name = next((re.match(r"    \.name:\s+(\S+)", x).group(1) for x in entry if re.match(r"    \.name:\s", x)), None)
        if name in res:
            res[name]["metadata"] = [x.rstrip() for x in entry]
    return res


def side(files, rev, extra, tmp):
    base = os.path.join(ROOT, CSRC)
    if rev:
        base = os.path.join(tempfile.mkdtemp(dir=tmp, prefix="rev"), CSRC)
        tar = subprocess.check_output(["git", "-C", ROOT, "archive", rev, CSRC, "include"])      # (the headers reach up to include/orbx.h)
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(os.path.dirname(os.path.dirname(base)))
    if not files:
        files = sorted(f for f in os.listdir(base) if f.endswith(".hip"))
    asm_dir = tempfile.mkdtemp(dir=tmp, prefix="asm")
    res = {}
    for f in files:
        for name, k in kernels(assembly(f if os.path.dirname(f) else os.path.join(base, f), extra, asm_dir)).items():
            assert name not in res, name + " defined twice on one side"
            res[name] = dict(k, file=os.path.basename(f))
    return res


def pretty(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, (re.sub(r"\(.*", "", o.replace("void ", "")) for o in out)))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", nargs="*", default=[], help=".hip files of side A")
    ap.add_argument("--b", nargs="*", default=[], help=".hip files of side B")
    ap.add_argument("--a-rev", help="take side A's csrc from this commit")
    ap.add_argument("--b-rev", help="take side B's csrc from this commit")
    ap.add_argument("--flags", action="append", default=[], help="extra compiler flag for both sides (repeatable), e.g. --flags=-DORBX_DIAG")
    ap.add_argument("--show", action="store_true", help="print the unified diff of what differs")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        A, B = side(args.a, args.a_rev, args.flags, tmp), side(args.b, args.b_rev, args.flags, tmp)
    names = sorted(set(A) | set(B))
    nice = pretty(names)
    bad = 0
    for n in names:
        if n not in A or n not in B:
            print(f"ONLY IN {'A' if n in A else 'B'}  {nice[n]}  ({(A.get(n) or B.get(n))['file']})")
            bad += 1
            continue
        diff = [p for p in ("text", "descriptor", "metadata") if A[n][p] != B[n][p]]
        where = A[n]["file"] if A[n]["file"] == B[n]["file"] else f"{A[n]['file']} -> {B[n]['file']}"
        print(f"{'DIFFERS (' + ', '.join(diff) + ')' if diff else 'identical'}  {nice[n]}  ({where}; {len(A[n]['text'])} lines)")
        bad += bool(diff)
        if args.show:
            for p in diff:
                sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(A[n][p], B[n][p], "A " + p, "B " + p, lineterm="", n=2))
    print(f"{len(names)} kernels, {bad} differ or are missing on one side")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
