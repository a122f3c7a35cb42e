#!/usr/bin/env python3
"""What lossy links cost (csrc/lossy.hip).

Runs bench.py's configuration (engine_config, spread message order) on one box,
alternating whole runs of the contexts of one process:
  flood    loss off: the planner's flood, bench.py's own run
  p=0      loss on with every arc open: k_expand_lossy doing the flood's work
           from frontier rows, with none of the planner's shortcuts
  p=0.1    a tenth of the lines dropped
  p=0.5    half of them dropped
Prints per leg ms per run (reset + run + finalize, as bench.py's step), rounds,
ms per round, rows gathered, arcs scanned and the share of the (peer, message)
cells reached, then the rounds of each leg side by side.  Asserts that the
p = 0 leg's coverage and per-round counters are the flood's.
--parent-tree DIR first times bench.py of DIR against this tree's, loss off, in
alternating child processes (job record and dumped outputs compared): the flood
must not have slowed down.
usage: loss_cost.py [--workload c4|c5] [--log2n N] [--steps 5] [--seed 11] [--out FILE]
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

LEGS = {"flood": None, "p=0": 0.0, "p=0.1": 0.1, "p=0.5": 0.5}


def engine(pkg, bench, args, p, seed):
    eng = pkg.GossipEngine(0, **bench.engine_config(args))
    eng.build_chung_lu(1 << args.log2n, args.dbar, args.gamma, args.seed)
    origin = pkg.overlay.random_origins(1 << args.log2n, args.messages, seed=args.seed)
    origin = origin[eng.spread_order(origin, hops=args.spread_hops)]
    eng.set_messages(origin)
    eng.link_loss(p, seed)
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
    say(f"{a.workload.upper()} 2^{args.log2n} x {args.messages}, bench.py's configuration, loss seed {a.seed}, "
        f"{a.steps} runs per leg")
    engs = {k: engine(pkg, bench, args, p, a.seed) for k, p in LEGS.items()}
    ms = {k: [] for k in LEGS}
    last = {}
    for e in engs.values():
        step(e)   # warm-up
    for _ in range(a.steps):
        for k, e in engs.items():
            t, last[k] = step(e)
            ms[k].append(t)
    cells = float(1 << args.log2n) * float(args.messages)
    cov = {k: e.coverage() for k, e in engs.items()}
    flood_ms = float(np.median(ms["flood"]))
    for k in LEGS:
        st = last[k]
        modes = sorted({s["mode"] for s in st})
        say(f"{k:6s}: ms per run {span(ms[k])} ({np.median(ms[k]) / flood_ms:.2f} x the flood); {len(st)} rounds, "
            f"{np.median(ms[k]) / len(st):.2f} ms per round; rows gathered {sum(s['rows_gathered'] for s in st)}, "
            f"arcs scanned {sum(s['arcs_scanned'] for s in st)}, row bytes {sum(s['row_bytes'] for s in st) / 1e9:.2f} GB; "
            f"reached {100.0 * float(cov[k].sum()) / cells:.2f} % of the cells; modes {modes}")
    assert np.array_equal(cov["flood"], cov["p=0"]), "every arc open: coverage differs from the flood's"
    assert len(last["flood"]) == len(last["p=0"])
    for x, y in zip(last["flood"], last["p=0"]):
        for key in ("injected", "new_bits", "receivers", "sends", "active"):
            assert x[key] == y[key], (key, x["round"], x[key], y[key])
    say("every arc open: coverage and the per-round counters are the flood's")
    say("round  " + "  ".join(f"{k + ' ms':>10s} {'new bits':>12s}" for k in LEGS))
    for r in range(max(len(s) for s in last.values())):
        say(f"{r:5d}  " + "  ".join(f"{last[k][r]['round_ms']:10.3f} {last[k][r]['new_bits']:12d}" if r < len(last[k])
                                   else " " * 23 for k in LEGS))
    for e in engs.values():
        e.close()
    flush()


if __name__ == "__main__":
    main()
