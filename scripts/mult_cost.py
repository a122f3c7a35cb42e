#!/usr/bin/env python3
"""What the delivery multiplicity record costs (csrc/mult.hip).

Runs bench.py's configuration (engine_config, spread message order) on the
same box, alternating whole runs of three contexts of one process: untracked,
with gp_track_fresh (the yardstick: the same gather, one popcount per arc) and
with gp_track_mult.  Prints ms per run (reset + run + finalize, as bench.py's
step) and, per round, the two passes -- round_ms - expand_ms against the
untracked run's -- side by side; then the cost of the four reads, the
histogram, and the headline table: fragility.by_degree(sole_bins()).  Asserts
the record's identities on the run: the histogram sums to the coverage and to
the rounds' new_bits, bin 1 is the sum of either sole array, the sole arrays
stay below the fresh ones, and the device table is fragility.bins of the
arrays read.
--parent-tree DIR first times bench.py of DIR against this tree's, untracked,
in alternating child processes.
usage: mult_cost.py [--workload c4|c5] [--log2n N] [--steps 5] [--out FILE] [--parent-tree DIR --pairs 3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from delay_cost import timed  # noqa: E402
from fresh_cost import bench_args, span, step  # noqa: E402


def engine(pkg, bench, args, record):
    eng = pkg.GossipEngine(0, **bench.engine_config(args))
    eng.build_chung_lu(1 << args.log2n, args.dbar, args.gamma, args.seed)
    origin = pkg.overlay.random_origins(1 << args.log2n, args.messages, seed=args.seed)
    origin = origin[eng.spread_order(origin, hops=args.spread_hops)]
    eng.set_messages(origin)
    if record:
        getattr(eng, "track_" + record)()
    eng.reset()
    return eng


def pass_table(say, st_mult, st_fresh, st_off):
    say("pass per round = (round_ms - expand_ms) less the untracked run's: gp_track_mult beside gp_track_fresh")
    say("round     active  receivers   mult ms  fresh ms  expand_ms   mult / fresh")
    tm = tf = 0.0
    for a, f, b in zip(st_mult, st_fresh, st_off):
        base = b["round_ms"] - b["expand_ms"]
        ms = (a["round_ms"] - a["expand_ms"]) - base
        fs = (f["round_ms"] - f["expand_ms"]) - base
        tm += ms
        tf += fs
        say(f"{a['round']:5d} {a['active']:10d} {a['receivers']:10d} {ms:9.3f} {fs:9.3f} {a['expand_ms']:10.3f} "
            f"{ms / max(fs, 1e-6):10.2f}")
    say(f"the passes of a run sum to {tm:.2f} ms (mult) and {tf:.2f} ms (fresh)")


def report(say, pkg, eng, fresh_eng, stats):
    t_hist, hist = timed(eng, eng.mult_hist)
    t_recv, recv = timed(eng, eng.sole_recv)
    t_sent, sent = timed(eng, eng.sole_sent)
    t_bins, table = timed(eng, eng.sole_bins)
    t_bins2, _ = timed(eng, eng.sole_bins)
    sp, deg = eng.seenpop(), eng.degrees()
    say(f"read of mult_hist {t_hist:.2f} ms, of sole_recv {t_recv:.2f} ms ({recv.nbytes / 1e6:.0f} MB), of sole_sent "
        f"{t_sent:.2f} ms ({sent.nbytes / 1e6:.0f} MB); gp_read_sole_bins {t_bins:.2f} ms, again {t_bins2:.2f} ms")
    h = hist.astype(np.int64)
    assert int(h.sum()) == int(eng.coverage().sum(dtype=np.int64)), "the histogram does not sum to the coverage"
    assert int(h[1:].sum()) == sum(s["new_bits"] for s in stats), "bins 1 .. 16 are not the rounds' new_bits"
    assert int(h[0]) == sum(s["injected"] for s in stats), "bin 0 is not the injections"
    assert int(h[1]) == int(recv.sum(dtype=np.int64)) == int(sent.sum(dtype=np.int64)), "bin 1 is not the sole arrays' sum"
    assert np.array_equal(table, pkg.fragility.bins(deg, sp, recv, sent)), "the device table is not the arrays'"
    fr, fs = fresh_eng.fresh_recv(), fresh_eng.fresh_sent()
    assert (recv <= fr).all() and (sent <= fs).all(), "a sole count above the fresh count"
    weighted = sum(c * int(h[c]) for c in range(1, 17))
    assert weighted <= int(fr.sum(dtype=np.int64)), "the histogram's deliveries exceed fresh_recv"
    say("deliverers " + " ".join(f"{c:>9d}" for c in range(16)) + "       16+")
    say("receipts   " + " ".join(f"{int(x):>9d}" for x in h))
    say(f"sole share of the expansion's receipts {pkg.fragility.sole_share(hist):.4f}; with 2 or more deliverers "
        f"{pkg.fragility.at_least(hist, 2)}, with 16 or more {pkg.fragility.at_least(hist, 16)}; mean deliverers per "
        f"receipt {int(fr.sum(dtype=np.int64)) / max(int(h[1:].sum()), 1):.3f}; largest sole_sent {int(sent.max())}")
    say("bin   degrees           peers     receipts  sole share  sole sent / peer  share of sole sent")
    for r in pkg.fragility.by_degree(table):
        say(f"{r['bin']:3d} {r['deg_lo']:8d}-{r['deg_hi']:<8d} {r['peers']:9d} {r['receipts']:12d} {r['sole_share']:11.4f} "
            f"{r['sole_per_peer']:17.2f} {r['sent_share']:19.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("c4", "c5"), default="c4")
    ap.add_argument("--log2n", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5)
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
    say(f"{a.workload.upper()} 2^{args.log2n} x {args.messages}, bench.py's configuration, {a.steps} runs per leg")
    legs = {"untracked": None, "fresh": "fresh", "mult": "mult"}
    engs = {k: engine(pkg, bench, args, v) for k, v in legs.items()}
    ms = {k: [] for k in legs}
    last = {}
    for e in engs.values():
        step(e)   # warm-up
    for _ in range(a.steps):
        for k, e in engs.items():
            t, last[k] = step(e)
            ms[k].append(t)
    for k in legs:
        say(f"{k:9s}: ms per run {span(ms[k])}; sum of round_ms {sum(s['round_ms'] for s in last[k]):.2f}")
    pass_table(say, last["mult"], last["fresh"], last["untracked"])
    flush()
    report(say, pkg, engs["mult"], engs["fresh"], last["mult"])
    flush()
    for e in engs.values():
        e.close()


if __name__ == "__main__":
    main()
