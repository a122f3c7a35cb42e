#!/usr/bin/env python3
"""Per-kernel diff of two directories of gfx950 device assembly (the check
that a refactor left every kernel's machine code alone).

Each directory holds one .s per csrc/*.hip, compiled with build_lib.FLAGS plus
`--cuda-device-only -S`.  For every kernel symbol (one with an .amdhsa_kernel
descriptor) the text from its .globl line to its .end_amdhsa_kernel -- code,
register counts, LDS and scratch sizes -- is compared, whichever unit holds it;
the function's index in its unit (.LBB<k>_<n> labels) is renumbered away and
the .amdgpu_metadata at the end of a unit is not looked at.
usage: isa_diff.py <dir_a> <dir_b> [-v]     exit status 1 if anything differs"""
import difflib
import glob
import os
import re
import sys


def kernels(directory):
    """symbol -> sorted texts (a weak template kernel may sit in several units)"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        start = {}
        for i, line in enumerate(lines):
            m = re.match(r"\s*\.(globl|weak)\s+(\S+)", line)
            if m:
                start.setdefault(m.group(2), i)
                continue
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if not m:
                continue
            sym = m.group(1)
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            text = "\n".join(lines[start.pop(sym):end + 1])
            text = re.sub(r"\.L(BB|JTI|CPI|tmp)\d+_", r".L\1_", text)
            text = re.sub(r"\bBB\d+_(\d+)", r"BB_\1", text)   # (the loop comments name blocks too)
            text = re.sub(r"[ \t]+", " ", text)               # (comment columns move with a label's width)
            out.setdefault(sym, []).append(text)
    return {s: sorted(t) for s, t in out.items()}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    verbose = "-v" in sys.argv[3:]
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = [s for s in sorted(set(a) & set(b)) if a[s] != b[s]]
    for s in only_a:
        print(f"only in {sys.argv[1]}: {s}")
    for s in only_b:
        print(f"only in {sys.argv[2]}: {s}")
    for s in differ:
        print(f"differs: {s}")
        if verbose:
            d = difflib.unified_diff(a[s][0].split("\n"), b[s][0].split("\n"), "a", "b", lineterm="", n=2)
            print("\n".join(list(d)[:80]))
    print(f"kernels: {len(a)} in a, {len(b)} in b, compared {len(set(a) & set(b))}, differing {len(differ)}, "
          f"only in a {len(only_a)}, only in b {len(only_b)}")
    return 1 if differ or only_a or only_b else 0


if __name__ == "__main__":
    sys.exit(main())
