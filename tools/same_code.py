#!/usr/bin/env python3
"""Do two trees compile to the same device code?   tools/same_code.py PARENT_TREE BRANCH_TREE [--debug]

For every csrc/*.hip of either tree: the Makefile's flags plus `--cuda-device-only -S` (and -DVLPET_DEBUG with --debug), the
listing split per symbol -- the function body up to .Lfunc_end, its .amdhsa_kernel descriptor and its entry of the amdhsa.kernels
metadata -- comments and .loc / .file lines dropped, the compiler's label counters normalised, and the texts compared.  Prints the
per-object table (kernels before -> after, removed, added, differing) and the symbols behind every non-zero cell; exit status 1
if any cell but the counts is non-zero.  The script only diffs two listings: it knows nothing about any instruction.

--work DIR keeps the listings (DIR/parent[_dbg]/x.s, DIR/branch[_dbg]/x.s) and reuses one that is newer than its .hip and every
header of its tree; --objects a.hip b.hip restricts the run; --show prints a unified diff of each differing symbol.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("vl-pet_amd", "csrc")


def makefile_flags(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS := (.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def listing(csrc, name, out, debug):
    src = os.path.join(csrc, name)
    deps = [src] + [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(p) for p in deps):
        return out
    cmd = ["hipcc"] + makefile_flags(csrc) + (["-DVLPET_DEBUG"] if debug else []) + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("%s\n%s" % (" ".join(cmd), r.stderr))
    return out


LABELS = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Ltmp\d+"), ".Ltmp"),
          (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1")]


def clean(line):
    line = line.split(";", 1)[0].rstrip()                   # comments (no string of a device listing holds a ';')
    if not line.strip() or re.match(r"\s*\.(loc|file)\s", line):
        return None
    for pat, to in LABELS:
        line = pat.sub(to, line)
    return line


def symbols(path):
    """({symbol: text}, kernels) -- every function of a listing: its body from the label to .Lfunc_end (the .amdhsa_kernel
    descriptor lies in between) and, for a kernel, its entry of the amdhsa.kernels metadata"""
    lines = open(path).read().split("\n")
    out, kern, name = {}, set(), None
    for i, l in enumerate(lines):
        m = re.match(r"([^\s:]+):", l)
        if name is None:
            if m and i and lines[i - 1].split() == [".type", m.group(1) + ",@function"]:
                name = m.group(1)
                out[name] = [l]
            continue
        out[name].append(l)
        if l.split()[:1] == [".amdhsa_kernel"]:
            kern.add(name)
        if m and m.group(1).startswith(".Lfunc_end"):
            name = None
    # amdhsa.kernels is a YAML list: an entry starts at "  - " and names its kernel under .name
    k0 = next((k for k, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines))
    entry = []
    for l in lines[k0 + 1:] + ["end"]:
        if entry and not l.startswith("   "):
            nm = next(e.split()[1] for e in entry if e.split()[:1] == [".name:"])
            out[nm] += entry
            entry = []
        if not l.startswith("  "):
            break
        entry.append(l)
    return {k: "\n".join(c for c in map(clean, v) if c is not None) for k, v in out.items()}, kern


def demangle(names):
    if not names:
        return {}
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
        return dict(zip(names, r.stdout.split("\n")))
    except OSError:
        return {x: x for x in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent"), ap.add_argument("branch")
    ap.add_argument("--debug", action="store_true", help="add -DVLPET_DEBUG (the diagnosis library)")
    ap.add_argument("--work", help="keep and reuse listings under this directory")
    ap.add_argument("--objects", nargs="*", help="only these .hip files")
    ap.add_argument("--show", action="store_true", help="print a diff of every differing symbol")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="same_code_")
    sides = {"parent": os.path.join(a.parent, CSRC), "branch": os.path.join(a.branch, CSRC)}
    files = {s: sorted(f for f in os.listdir(c) if f.endswith(".hip")) for s, c in sides.items()}
    names = sorted(set(files["parent"]) | set(files["branch"]))
    if a.objects:
        names = [x for x in names if x in a.objects]
    jobs = {}
    with ThreadPoolExecutor(a.j) as ex:
        for s, c in sides.items():
            d = os.path.join(work, s + ("_dbg" if a.debug else ""))
            os.makedirs(d, exist_ok=True)
            for f in names:
                if f in files[s]:
                    jobs[s, f] = ex.submit(listing, c, f, os.path.join(d, f[:-4] + ".s"), a.debug)
    print("| object | kernels before → after | removed | added | differing |\n|---|---|---|---|---|")
    tot = [0, 0, 0, 0, 0]
    detail = []
    for f in names:
        sy, kn = {}, {}
        for s in sides:
            p = jobs[s, f].result() if (s, f) in jobs else None
            sy[s], kn[s] = symbols(p) if p else ({}, set())
        removed = sorted(set(sy["parent"]) - set(sy["branch"]))
        added = sorted(set(sy["branch"]) - set(sy["parent"]))
        differing = sorted(k for k in set(sy["parent"]) & set(sy["branch"]) if sy["parent"][k] != sy["branch"][k])
        row = [len(kn["parent"]), len(kn["branch"]), len(removed), len(added), len(differing)]
        tot = [x + y for x, y in zip(tot, row)]
        print("| `%s` | %d → %d | %d | %d | %d |" % (f, *row))
        dm = demangle(removed + added + differing)
        for what, lst in (("removed", removed), ("added", added), ("differing", differing)):
            detail += ["%s: %s `%s`" % (f, what, dm.get(k, k)) for k in lst]
        if a.show:
            for k in differing:
                detail += list(difflib.unified_diff(sy["parent"][k].split("\n"), sy["branch"][k].split("\n"),
                                                    "parent " + k, "branch " + k, lineterm="", n=2))
    print("| **all** | **%d → %d** | %d | %d | %d |" % tuple(tot))
    print("\n".join(detail))
    return 1 if any(tot[2:]) else 0


if __name__ == "__main__":
    sys.exit(main())
