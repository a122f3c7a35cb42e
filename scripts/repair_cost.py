#!/usr/bin/env python3
"""What anti-entropy repair buys and costs (csrc/repair.hip).

Runs bench.py's configuration (engine_config, spread message order) on one box,
alternating whole runs of the contexts of one process, in three groups by link
setting -- the flood, link_loss(0.1), link_loss(0.5) -- each with three legs:
no repair, repair at period 1 and at period 4.  A run with repair stops after
`period` silent rounds, which one random partner per round seldom reaches
early; every run is cut at --max-rounds (32) rounds, and the table says which
legs the cut ended.
Prints per leg ms per run (reset + run + finalize, as bench.py's step), rounds,
the median ms of a repair round and of a non-repair round (round_ms of the last
run), exchanges and lines carried, and the share of the (peer, message) cells
reached; then the rounds of each leg side by side.  Asserts that without loss
the legs with repair reach exactly the flood's coverage.
--parent-tree DIR first times bench.py of DIR against this tree's, repair off,
in alternating child processes (job record and dumped outputs compared): the
flood must not have slowed down.
usage: repair_cost.py [--workload c4|c5] [--log2n N] [--steps 3] [--max-rounds 32] [--seed 21] [--loss-seed 11]
                      [--out FILE] [--parent-tree DIR --pairs 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fresh_cost import bench_args, span  # noqa: E402

LINKS = [("flood", None), ("loss 0.1", 0.1), ("loss 0.5", 0.5)]
PERIODS = (0, 1, 4)


def engine(pkg, bench, args, p, period, a):
    eng = pkg.GossipEngine(0, **bench.engine_config(args))
    eng.build_chung_lu(1 << args.log2n, args.dbar, args.gamma, args.seed)
    origin = pkg.overlay.random_origins(1 << args.log2n, args.messages, seed=args.seed)
    origin = origin[eng.spread_order(origin, hops=args.spread_hops)]
    eng.set_messages(origin)
    if p is not None:
        eng.link_loss(p, a.loss_seed)
    if period:
        eng.repair(period, a.seed)
    eng.reset()
    return eng


def step(eng, max_rounds):
    eng.synchronize()
    t0 = time.perf_counter()
    eng.reset()
    st = eng.run(max_rounds)
    eng.finalize()
    eng.synchronize()
    return (time.perf_counter() - t0) * 1e3, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("c4", "c5"), default="c4")
    ap.add_argument("--log2n", type=int, default=0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--max-rounds", type=int, default=32)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--loss-seed", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--pairs", type=int, default=5)
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
    cells = float(1 << args.log2n) * float(args.messages)
    say(f"{a.workload.upper()} 2^{args.log2n} x {args.messages}, bench.py's configuration, loss seed {a.loss_seed}, "
        f"repair seed {a.seed}, {a.steps} runs per leg, every run cut at {a.max_rounds} rounds")
    flood_cov = None
    for link, p in LINKS:
        names = [f"{link}, " + (f"period {k}" if k else "no repair") for k in PERIODS]
        engs = {n: engine(pkg, bench, args, p, k, a) for n, k in zip(names, PERIODS)}
        ms = {n: [] for n in names}
        last = {}
        for e in engs.values():
            step(e, a.max_rounds)   # warm-up
        for _ in range(a.steps):
            for n, e in engs.items():
                t, last[n] = step(e, a.max_rounds)
                ms[n].append(t)
        for n, k in zip(names, PERIODS):
            st, e = last[n], engs[n]
            cov = e.coverage()
            if flood_cov is None:
                flood_cov = cov
            if p is None:
                assert np.array_equal(cov, flood_cov), f"{n}: coverage differs from the flood's"
            rec = e.repair_record() if k else np.zeros((len(st), 2), np.uint64)
            kind = np.array([bool(k) and (s["round"] + 1) % k == 0 for s in st])
            rms = np.array([s["round_ms"] for s in st])
            rep = f"{np.median(rms[kind]):.2f}" if kind.any() else "-"
            non = f"{np.median(rms[~kind]):.2f}" if (~kind).any() else "-"
            cut = len(st) == a.max_rounds and (st[-1]["new_bits"] > 0 or (k and e.repair_info()[3] < k))
            say(f"{n:22s}: ms per run {span(ms[n])}; {len(st)} rounds{' (cut)' if cut else ''}; ms per repair round {rep}, "
                f"per other round {non}; exchanges {int(rec[:, 0].sum())}, lines {int(rec[:, 1].sum())}; "
                f"cells reached {float(cov.sum()) / cells:.4f}; modes {sorted({s['mode'] for s in st})}")
        if p is None:
            say("without loss the legs with repair reach the flood's coverage exactly")
        say("round  " + "  ".join(f"{('p' + str(k) if k else 'none') + ' ms':>9s} {'new bits':>12s} {'lines':>12s}" for k in PERIODS))
        recs = {n: (engs[n].repair_record() if k else None) for n, k in zip(names, PERIODS)}
        for r in range(max(len(s) for s in last.values())):
            say(f"{r:5d}  " + "  ".join(
                f"{last[n][r]['round_ms']:9.3f} {last[n][r]['new_bits']:12d} {int(recs[n][r, 1]) if recs[n] is not None else 0:12d}"
                if r < len(last[n]) else " " * 35 for n in names))
        for e in engs.values():
            e.close()
        flush()


if __name__ == "__main__":
    main()
