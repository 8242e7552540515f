#!/usr/bin/env python3
"""Compare the gfx950 device assembly of translation units between two source trees, kernel by kernel.

    scripts/compare_kernel_isa.py PARENT HEAD conv_igemm.hip conv_wgrad.hip ...

PARENT and HEAD are git revisions, or directories that hold a text2video_amd/csrc tree (`.` is the working tree).  Each file
of text2video_amd/csrc is compiled on both sides with the Makefile's CXXFLAGS plus `--cuda-device-only -S`; no GPU is needed.
Per kernel symbol the script prints "identical", or both sides' code-object metadata and the number of differing lines.  It
compares the two texts and nothing else.  The per-file `__hip_cuid_*` symbol is a hash of the source text and is left out.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("text2video_amd", "csrc")
META = ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "kernarg_segment_size")


def makefile_flags(tree):
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def checkout(rev, tmp):
    """The tree of `rev`: the directory itself, or `git archive` of the revision's csrc and include."""
    if os.path.isdir(os.path.join(rev, CSRC)):
        return os.path.abspath(rev)
    dst = os.path.join(tmp, re.sub(r"\W", "_", rev))
    os.makedirs(dst)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], check=True, stdout=subprocess.PIPE).stdout
    subprocess.run(["tar", "-x", "-C", dst], input=tar, check=True)
    return dst


def assemble(tree, name, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + makefile_flags(tree) + ["--cuda-device-only", "-S", name, "-o", out], check=True,
                   cwd=os.path.join(tree, CSRC), stderr=subprocess.DEVNULL)
    return [l for l in open(out).read().splitlines() if "__hip_cuid_" not in l]


def kernels(lines):
    """{symbol: (text lines from the entry label to .end_amdhsa_kernel, metadata dict)}, and the lines outside any kernel."""
    out, rest, i = {}, [], 0
    names = [m.group(1) for m in (re.match(r"\s+\.amdhsa_kernel (\S+)", l) for l in lines) if m]
    starts = {n + ":" for n in names}
    while i < len(lines):
        head = lines[i].split(" ", 1)[0].split("\t", 1)[0]
        if head in starts:
            j = i
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            out[head[:-1]] = [lines[i:j + 1], {}]
            i = j + 1
        else:
            rest.append(lines[i])
            i += 1
    # the YAML notes at the end: one record per kernel, keys sorted, so .name follows the record's first fields
    rec = {}
    for l in lines:
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)\s*$", l)
        if not m:
            continue
        if l.lstrip().startswith("- .agpr_count"):
            rec = {}
        rec[m.group(1)] = m.group(2)
        if m.group(1) == "vgpr_spill_count" and rec.get("name") in out:
            out[rec["name"]][1] = {k: rec.get(k) for k in META}
    return out, rest


def differing(a, b):
    return sum(1 for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    parent, head, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    same = True
    with tempfile.TemporaryDirectory() as tmp:
        trees = [checkout(parent, tmp), checkout(head, tmp)]
        jobs = [(t, f, os.path.join(tmp, "%d_%s.s" % (s, f))) for f in files for s, t in enumerate(trees)]
        with ThreadPoolExecutor(max_workers=min(len(jobs), 8)) as pool:
            texts = list(pool.map(lambda j: assemble(*j), jobs))
        for n, f in enumerate(files):
            (ka, ra), (kb, rb) = kernels(texts[2 * n]), kernels(texts[2 * n + 1])
            print("%s: %d kernels at %s, %d at %s" % (f, len(ka), parent, len(kb), head))
            for sym in sorted(set(ka) | set(kb)):
                if sym not in ka or sym not in kb:
                    print("  %s: only at %s" % (sym, parent if sym in ka else head))
                    same = False
                elif ka[sym][0] == kb[sym][0] and ka[sym][1] == kb[sym][1]:
                    print("  %s: identical (%d lines)" % (sym, len(ka[sym][0])))
                else:
                    same = False
                    print("  %s: %d of %d lines differ" % (sym, differing(ka[sym][0], kb[sym][0]), len(ka[sym][0])))
                    for side, k in ((parent, ka), (head, kb)):
                        print("    %-8s %s" % (side, " ".join("%s=%s" % (m, k[sym][1].get(m)) for m in META)))
            d = differing(ra, rb)
            same = same and d == 0
            print("  outside the kernels: %s" % ("identical" if d == 0 else "%d lines differ" % d))
    print("all identical" if same else "not identical")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
