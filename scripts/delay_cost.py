#!/usr/bin/env python3
"""What the per-peer receipt-delay record costs (csrc/delay.hip).

Runs bench.py's configuration (engine_config, spread message order) on the
same box, alternating whole runs, in two groups of contexts of one process:
  uniform  bench.py's own table (every message injected in round 0): untracked,
           tracked (k_delay_uniform: the guard words alone, no frontier rows),
           and tracked with GP_DELAY_ROWS=1 (k_delay<W> on the same run);
  general  the same origins with inject = k % 3: untracked and tracked
           (k_delay<W>, the receivers' own new rows).
Prints ms per run (reset + run + finalize, as bench.py's step) and, per round,
the pass -- round_ms - expand_ms against the untracked run's -- beside its
byte model: 4 B per owned vertex for the guard sweep, 5 B read and 5 B written
per receiver, and on the row path 8 W B per receiver; the achieved bytes/s
stand beside the ceilings of random rows DESIGN.md §6 cites (10.5 G random
512-B rows/s = 5.4 TB/s, 51 G random 64-B rows/s = 3.3 TB/s).  Then the cost
of gp_read_delay_bins and of reading the two arrays, and the headline table:
latency.by_degree(delay_bins()).  Asserts that the two paths agree on the
uniform table, that the device table is latency.bins of the arrays read, and
that the record's sum is the rounds' receipts weighted by their delay.
--parent-tree DIR first times bench.py of DIR against this tree's, untracked,
in alternating child processes.
usage: delay_cost.py [--workload c4|c5] [--log2n N] [--steps 5] [--out FILE] [--parent-tree DIR --pairs 3]
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

ROW_CEILING = {64: 10.5e9 * 512, 8: 51e9 * 64}   # bytes/s of random 512-B and 64-B rows


def engine(pkg, bench, args, inject, track, rows=False):
    if rows:   # read at gp_create
        os.environ["GP_DELAY_ROWS"] = "1"
    eng = pkg.GossipEngine(0, **bench.engine_config(args))
    os.environ.pop("GP_DELAY_ROWS", None)
    eng.build_chung_lu(1 << args.log2n, args.dbar, args.gamma, args.seed)
    origin = pkg.overlay.random_origins(1 << args.log2n, args.messages, seed=args.seed)
    origin = origin[eng.spread_order(origin, hops=args.spread_hops)]
    eng.set_messages(origin, inject)
    eng.track_delay(track)
    eng.reset()
    return eng


def timed(eng, fn):
    eng.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def pass_table(say, name, st_on, st_off, n, words, rows):
    """the pass per round: (round_ms - expand_ms) tracked less untracked, and its byte model"""
    say(f"{name}: pass per round = (round_ms - expand_ms) less the untracked run's; model = 4 B x {n} vertices + "
        f"10 B x receivers" + (f" + {8 * words} B x receivers" if rows else ""))
    say("round     active  receivers   pass ms  expand_ms   model MB   model GB/s")
    tot = 0.0
    for a, b in zip(st_on, st_off):
        ms = (a["round_ms"] - a["expand_ms"]) - (b["round_ms"] - b["expand_ms"])
        tot += ms
        model = 4 * n + (10 + (8 * words if rows else 0)) * a["receivers"]
        say(f"{a['round']:5d} {a['active']:10d} {a['receivers']:10d} {ms:9.3f} {a['expand_ms']:10.3f} "
            f"{model / 1e6:10.1f} {model / 1e6 / max(ms, 1e-6):12.1f}")
    say(f"{name}: the passes of a run sum to {tot:.2f} ms")
    if rows:
        ceil = ROW_CEILING[64 if words == 64 else 8]
        say(f"  (ceiling of random {8 * words}-B rows: {ceil / 1e12:.1f} TB/s)")


def report(say, pkg, eng, stats, inject):
    t_sum, dsum = timed(eng, eng.delay_sum)
    t_max, dmax = timed(eng, eng.delay_max)
    t_bins, table = timed(eng, eng.delay_bins)
    t_bins2, _ = timed(eng, eng.delay_bins)
    sp, deg = eng.seenpop(), eng.degrees()
    assert np.array_equal(table, pkg.latency.bins(deg, sp, dsum, dmax)), "the device table is not the arrays'"
    say(f"read of delay_sum {t_sum:.2f} ms ({dsum.nbytes / 1e6:.0f} MB), of delay_max {t_max:.2f} ms "
        f"({dmax.nbytes / 1e6:.0f} MB); gp_read_delay_bins {t_bins:.2f} ms, again {t_bins2:.2f} ms (1.3 KB to the host)")
    if inject is None:
        want = sum((s["round"] + 1) * s["new_bits"] for s in stats)
        assert int(dsum.sum(dtype=np.int64)) == want, "the record's sum is not the receipts weighted by their round"
    say(f"receipts {int(sp.sum(dtype=np.int64))}, sum of delays {int(dsum.sum(dtype=np.int64))}, "
        f"largest delay {int(dmax.max())}, peers never reached {int((sp == 0).sum())}")
    say("bin   degrees           peers    reach   mean delay   max delay")
    for r in pkg.latency.by_degree(table):
        say(f"{r['bin']:3d} {r['deg_lo']:8d}-{r['deg_hi']:<8d} {r['peers']:9d} {r['reach']:8.4f} {r['mean_delay']:12.4f} "
            f"{r['max_delay']:11d}")
    return dsum, dmax


def group(say, pkg, bench, args, a, name, inject, legs):
    """legs: {label: (track, rows)}; alternating runs of the contexts of one group"""
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
    n, words = engs["untracked"].n, engs["untracked"].words
    out = {}
    for k, (track, rows) in legs.items():
        if track:
            pass_table(say, f"{name} {k}", last[k], last["untracked"], n, words, rows or inject is not None)
            out[k] = report(say, pkg, engs[k], last[k], inject)
    for e in engs.values():
        e.close()
    return out


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
    got = group(say, pkg, bench, args, a, "uniform", None,
                {"untracked": (False, False), "tracked": (True, False), "rows": (True, True)})
    assert all(np.array_equal(x, y) for x, y in zip(got["tracked"], got["rows"])), "the two paths disagree"
    say("uniform: the guard-word path and the row path (GP_DELAY_ROWS=1) gave identical arrays")
    flush()
    inject = (np.arange(args.messages) % 3).astype(np.int32)
    say("general: the same origins, inject = k % 3")
    group(say, pkg, bench, args, a, "general", inject, {"untracked": (False, False), "tracked": (True, False)})
    flush()


if __name__ == "__main__":
    main()
