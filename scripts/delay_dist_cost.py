#!/usr/bin/env python3
"""What the per-peer delay distributions cost (csrc/delay_dist.hip, DESIGN.md
§3.16), beside the receipt delays' own passes (csrc/delay.hip) on the same runs.

Runs bench.py's configuration (engine_config, spread message order) on one box,
alternating whole runs, in groups of contexts of one process:
  uniform  bench.py's own table (every message injected in round 0): untracked,
           `delay` (k_delay_uniform) and `dist` (k_delay_dist_uniform), both the
           guard words alone, no frontier rows;
  rows     the same table with GP_DELAY_ROWS=1: untracked, `delay` (k_delay<W>)
           and `dist` (k_delay_dist<W>);
  general  the same origins with inject = k % 3: the same three legs.
Prints ms per run (reset + run + finalize, as bench.py's step) and, per round,
each leg's pass -- round_ms - expand_ms against the untracked run's -- the
ratio of the dist pass to the delay pass, and every leg's expand_ms (a tracked
run's expansion also stores the frontier rows the untracked run does not keep).
Then the cost of the reads and the headline table: p50 / p90 / p99 of the delays
by degree bin (latency.dist_by_degree(delay_dist_bins())).  Asserts that every leg of a table
gives the same array, that the device table is latency.dist_bins of the array
read, and that every row sums to seenpop.
--parent-tree DIR first times bench.py of DIR against this tree's, untracked,
in alternating child processes (job record and dumped outputs compared).
usage: delay_dist_cost.py [--workload c4|c5] [--log2n N] [--steps 5] [--out FILE] [--parent-tree DIR --pairs 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fresh_cost import bench_args, span, step  # noqa: E402

LEVERS = ("GP_DELAY_ROWS",)


def engine(pkg, bench, args, inject, record, env):
    for k in LEVERS:   # read at gp_create
        os.environ.pop(k, None)
    os.environ.update(env)
    eng = pkg.GossipEngine(0, **bench.engine_config(args))
    for k in LEVERS:
        os.environ.pop(k, None)
    eng.build_chung_lu(1 << args.log2n, args.dbar, args.gamma, args.seed)
    origin = pkg.overlay.random_origins(1 << args.log2n, args.messages, seed=args.seed)
    origin = origin[eng.spread_order(origin, hops=args.spread_hops)]
    eng.set_messages(origin, inject)
    eng.track_delay(record == "delay")
    eng.track_delay_dist(record == "dist")
    eng.reset()
    return eng


def timed(eng, fn):
    eng.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def passes(st_on, st_off):
    return [(a["round_ms"] - a["expand_ms"]) - (b["round_ms"] - b["expand_ms"]) for a, b in zip(st_on, st_off)]


def pass_table(say, name, last, legs):
    tracked = [k for k in legs if k != "untracked"]
    per = {k: passes(last[k], last["untracked"]) for k in tracked}
    say(f"{name}: pass per round = (round_ms - expand_ms) less the untracked run's, ms")
    say("round     active  receivers " + " ".join(f"{k:>9s}" for k in tracked) + "   dist / delay   expand_ms: " +
        " ".join(f"{k:>9s}" for k in legs))
    for i, s in enumerate(last["untracked"]):
        ratio = per["dist"][i] / max(per["delay"][i], 1e-6)
        say(f"{s['round']:5d} {s['active']:10d} {s['receivers']:10d} " + " ".join(f"{per[k][i]:9.3f}" for k in tracked) +
            f" {ratio:14.2f}              " + " ".join(f"{last[k][i]['expand_ms']:9.3f}" for k in legs))
    say(f"{name}: the passes of a run sum to " + ", ".join(f"{k} {sum(per[k]):.2f} ms" for k in tracked) +
        f"; dist / delay = {sum(per['dist']) / max(sum(per['delay']), 1e-6):.2f}")


def report(say, pkg, eng):
    t_read, dist = timed(eng, eng.delay_dist)
    t_bins, table = timed(eng, eng.delay_dist_bins)
    t_bins2, _ = timed(eng, eng.delay_dist_bins)
    sp, deg = eng.seenpop(), eng.degrees()
    assert np.array_equal(table, pkg.latency.dist_bins(deg, dist)), "the device table is not the array's"
    pkg.latency.dist_check(dist, sp)
    say(f"read of delay_dist {t_read:.2f} ms ({dist.nbytes / 1e6:.0f} MB); gp_read_delay_dist_bins {t_bins:.2f} ms, "
        f"again {t_bins2:.2f} ms (4 KB to the host)")
    cols = dist.sum(axis=0, dtype=np.int64)
    say(f"receipts {int(cols.sum())}; per delay 0 .. 15+: " + " ".join(str(int(x)) for x in cols))
    say("bin   degrees          receipts   mean delay   p50   p90   p99")
    for r in pkg.latency.dist_by_degree(table):
        say(f"{r['bin']:3d} {r['deg_lo']:8d}-{r['deg_hi']:<8d} {r['receipts']:12d} {r['mean_delay']:10.4f} "
            f"{r['p50']:5d} {r['p90']:5d} {r['p99']:5d}" + ("  (saturated)" if r["saturated"] else ""))
    return dist


def group(say, pkg, bench, args, a, name, inject, legs):
    """legs: {label: (record, env)}; alternating runs of the contexts of one group"""
    engs = {k: engine(pkg, bench, args, inject, *v) for k, v in legs.items()}
    ms = {k: [] for k in legs}
    last = {}
    for e in engs.values():
        step(e)   # warm-up
    for _ in range(a.steps):
        for k, e in engs.items():
            t, last[k] = step(e)
            ms[k].append(t)
    for k in legs:
        say(f"{name} {k:9s}: ms per run {span(ms[k])}; sum of round_ms {sum(s['round_ms'] for s in last[k]):.2f}")
    pass_table(say, name, last, legs)
    out = [report(say, pkg, engs[k]) if k == "dist" else engs[k].delay_dist()
           for k, (record, _) in legs.items() if record == "dist"]
    assert all(np.array_equal(out[0], x) for x in out[1:]), "the legs disagree"
    for e in engs.values():
        e.close()
    return out[0]


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
    rows = {"GP_DELAY_ROWS": "1"}
    by_rows = {"untracked": (None, {}), "delay": ("delay", rows), "dist": ("dist", rows)}
    uniform = group(say, pkg, bench, args, a, "uniform", None,
                    {"untracked": (None, {}), "delay": ("delay", {}), "dist": ("dist", {})})
    flush()
    forced = group(say, pkg, bench, args, a, "rows", None, by_rows)
    assert np.array_equal(uniform, forced), "the two paths disagree"
    say("uniform, rows: the guard-word path and the row path (GP_DELAY_ROWS=1) gave identical arrays")
    flush()
    inject = (np.arange(args.messages) % 3).astype(np.int32)
    say("general: the same origins, inject = k % 3")
    group(say, pkg, bench, args, a, "general", inject, {k: (rec, {}) for k, (rec, _) in by_rows.items()})
    flush()


if __name__ == "__main__":
    main()
