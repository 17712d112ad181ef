#!/usr/bin/env python3
"""Which kernels' machine code differs between two checkouts (CPU only).

    python scripts/kernel_isa_diff.py PARENT_CHECKOUT [THIS_TREE]

Every csrc/*.hip of both trees is cross-compiled with the library's flags and
--cuda-device-only -S, once plain and once with -DRC_ROW_TIMING. Kernels are
matched by mangled name, whichever unit defines them, and compared by
  - the instruction stream, comments stripped and local labels normalised
    (.LBB<function index>_<n>: the index changes when a kernel moves), and
  - the .amdhsa_kernel block (VGPRs, SGPRs, LDS, scratch, kernarg size).
One line per kernel that moved to another unit or differs; exit status 1 if a
kernel differs or exists on one side only.
"""
import glob
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LABEL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")


def library_flags(tree):
    spec = importlib.util.spec_from_file_location("rc_build", os.path.join(tree, "rna_clique_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC, [f for f in mod.FLAGS if f != "-shared"]


def clean(line):
    return LABEL.sub(r".L\1\2", line.split(";")[0]).strip()


def kernels_of(asm):
    """{mangled name: (instructions, descriptor)} of one unit's assembly."""
    out, lines, i = {}, asm.split("\n"), 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        i += 1
        if not m:
            continue
        name, body, desc, part = m.group(1), [], [], None
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            s = clean(lines[i])
            i += 1
            if s == name + ":":
                part = body
            elif s.startswith(".amdhsa_kernel"):
                part = desc
            elif s.startswith((".section", ".end_amdhsa_kernel")):
                part = None
            elif s and part is not None:
                part.append(s)
        if desc:
            out[name] = ("\n".join(body), "\n".join(desc))
    return out


def compile_tree(tree, defines, tmp):
    hipcc, flags = library_flags(tree)
    csrc = os.path.join(tree, "rna_clique_amd", "csrc")
    units = sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*.hip")))

    def one(u):
        s = os.path.join(tmp, u + ".s")
        subprocess.run([hipcc, *flags, *defines, "--cuda-device-only", "-S", "-o", s, u], cwd=csrc, check=True,
                       capture_output=True)
        return u, kernels_of(open(s).read())

    found = {}
    with ThreadPoolExecutor(min(len(units), 16)) as ex:
        for u, ks in ex.map(one, units):
            for k, v in ks.items():
                found[k] = (u, *v)
    return found


def main():
    parent = sys.argv[1]
    head = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    bad = 0
    for build, defines in (("plain", []), ("RC_ROW_TIMING", ["-DRC_ROW_TIMING"])):
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            a, b = compile_tree(parent, defines, ta), compile_tree(head, defines, tb)
        same = 0
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                verdict = "only in " + ("parent" if k in a else "this tree")
            else:
                diffs = [w for w, x, y in (("instructions", a[k][1], b[k][1]), ("descriptor", a[k][2], b[k][2])) if x != y]
                verdict = "DIFFERENT " + "+".join(diffs) if diffs else "identical"
            same += verdict == "identical"
            where = " -> ".join(dict.fromkeys(t[k][0] for t in (a, b) if k in t))
            if verdict != "identical" or " -> " in where:   # (identical in the same unit: counted only)
                print(f"{build:14s} {verdict:24s} {where:28s} {k}")
        total = len(set(a) | set(b))
        print(f"{build}: {same} of {total} kernels identical")
        bad += total - same
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
