#!/usr/bin/env python3
"""Do two runs take the same variant in every round and compute the same run?

Compares the per-round lines of two `bench.py --profile-steps` runs (stderr,
or a profiles/*_rounds.jsonl) field by field, everything but the `*_ms`
timings: mode, scan, every counter.  With two bench result lines as well,
their whole-run records (per-round counts and output fingerprints).
usage: rounds_diff.py A.err B.err [A.json B.json]     exit status 1 on a difference"""
import json
import sys


def rounds(path):
    return [json.loads(l) for l in open(path) if l.startswith('{"round"')]


def main():
    a, b = rounds(sys.argv[1]), rounds(sys.argv[2])
    bad = 0
    if len(a) != len(b):
        print(f"rounds: {len(a)} against {len(b)}")
        bad += 1
    for ra, rb in zip(a, b):
        for k in sorted(set(ra) | set(rb)):
            if not k.endswith("_ms") and ra.get(k) != rb.get(k):
                print(f"round {ra.get('round')}: {k} {ra.get(k)} against {rb.get(k)}")
                bad += 1
    print(f"{len(a)} rounds, {bad} differing fields")
    if len(sys.argv) > 4:
        ja, jb = (json.loads(open(p).read())["config"]["job"] for p in sys.argv[3:5])
        same = ja == jb
        print("whole-run record (per-round counts, digest / coverage / forwards fingerprints):",
              "identical" if same else f"DIFFERENT\n{ja}\n{jb}", ja["digest_fp"], ja["coverage_fp"], ja["forwards_fp"])
        bad += 0 if same else 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
