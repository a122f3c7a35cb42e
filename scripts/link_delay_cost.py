#!/usr/bin/env python3
"""What delayed links cost (csrc/delayed.hip).

Runs bench.py's configuration (engine_config, spread message order) on one box,
alternating whole runs of the contexts of one process, in two groups (the ring
of a dmax = 4 context holds five frontier-row buffers: all five legs at once
would not fit beside each other at 2^24 x 4096):
  group 1   flood     delay and loss off: the planner's flood, bench.py's own run
            loss p=0  link_loss(0): k_expand_lossy doing the flood's work from
                      frontier rows -- the kernel the delayed one is read against
            dmax=1    link_delay(1): k_expand_delayed doing the same work through
                      the delay bytes, the ring and the per-round bitmaps
  group 2   flood, dmax=2, dmax=4
Prints per leg ms per run (reset + run + finalize, as bench.py's step), rounds,
ms per round, rows gathered, arcs scanned and row bytes, then the rounds of
each leg side by side.  Asserts that the loss p=0 and dmax=1 legs' coverage and
per-round counters are the flood's, and that every leg's coverage is.
--parent-tree DIR first times bench.py of DIR against this tree's, delay off, in
alternating child processes (job record and dumped outputs compared): the flood
must not have slowed down.
usage: link_delay_cost.py [--workload c4|c5] [--log2n N] [--steps 5] [--seed 11] [--out FILE]
                          [--parent-tree DIR --pairs 3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fresh_cost import bench_args, span, step  # noqa: E402

GROUPS = [("flood", "loss p=0", "dmax=1"), ("flood", "dmax=2", "dmax=4")]
COUNTERS = ("injected", "new_bits", "receivers", "sends", "active")


def engine(pkg, bench, args, leg, seed):
    eng = pkg.GossipEngine(0, **bench.engine_config(args))
    eng.build_chung_lu(1 << args.log2n, args.dbar, args.gamma, args.seed)
    origin = pkg.overlay.random_origins(1 << args.log2n, args.messages, seed=args.seed)
    origin = origin[eng.spread_order(origin, hops=args.spread_hops)]
    eng.set_messages(origin)
    if leg == "loss p=0":
        eng.link_loss(0.0, seed)
    elif leg.startswith("dmax="):
        eng.link_delay(int(leg[5:]), seed)
    eng.reset()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("c4", "c5"), default="c4")
    ap.add_argument("--log2n", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if a.parent_tree:   # (before this process opens the GPU: the children time alone)
        from fresh_curve_cost import against_parent
        against_parent(say, a, os.path.abspath(a.parent_tree))
        flush()
    import _gossip_pkg
    pkg = _gossip_pkg.load()
    bench, args = bench_args(a.workload, a.log2n)
    say(f"{a.workload.upper()} 2^{args.log2n} x {args.messages}, bench.py's configuration, delay seed {a.seed}, "
        f"{a.steps} runs per leg")
    for names in GROUPS:
        engs = {k: engine(pkg, bench, args, k, a.seed) for k in names}
        ms = {k: [] for k in names}
        last = {}
        for e in engs.values():
            step(e)   # warm-up
        for _ in range(a.steps):
            for k, e in engs.items():
                t, last[k] = step(e)
                ms[k].append(t)
        cov = {k: e.coverage() for k, e in engs.items()}
        flood_ms = float(np.median(ms["flood"]))
        for k in names:
            st = last[k]
            modes = sorted({s["mode"] for s in st})
            say(f"{k:8s}: ms per run {span(ms[k])} ({np.median(ms[k]) / flood_ms:.2f} x the flood); {len(st)} rounds, "
                f"{np.median(ms[k]) / len(st):.2f} ms per round; rows gathered {sum(s['rows_gathered'] for s in st)}, "
                f"arcs scanned {sum(s['arcs_scanned'] for s in st)}, "
                f"row bytes {sum(s['row_bytes'] for s in st) / 1e9:.2f} GB; modes {modes}")
            assert np.array_equal(cov[k], cov["flood"]), f"{k}: coverage differs from the flood's"
        for k in names:
            if k in ("loss p=0", "dmax=1"):
                assert len(last[k]) == len(last["flood"])
                for x, y in zip(last["flood"], last[k]):
                    for key in COUNTERS:
                        assert x[key] == y[key], (k, key, x["round"], x[key], y[key])
                say(f"{k}: coverage and the per-round counters are the flood's")
        say("every leg's coverage is the flood's")
        say("round  " + "  ".join(f"{k + ' ms':>12s} {'new bits':>12s}" for k in names))
        for r in range(max(len(s) for s in last.values())):
            say(f"{r:5d}  " + "  ".join(f"{last[k][r]['round_ms']:12.3f} {last[k][r]['new_bits']:12d}"
                                       if r < len(last[k]) else " " * 25 for k in names))
        for e in engs.values():
            e.close()
        flush()


if __name__ == "__main__":
    main()
