#!/usr/bin/env python3
"""What the per-peer traffic record costs (csrc/load.hip).

Runs bench.py's configuration (engine_config, spread message order) on the
same box, alternating whole runs:
  c4   untracked, tracked lazy (nothing per round: the totals are computed at
       the read) and tracked eager (GP_LOAD_EAGER=1: the per-round pass), three
       contexts of one process;
  c5   untracked and tracked (churn: eager by necessity), one context at a
       time (two 2^26 x 4096 contexts do not fit beside each other).
Prints ms per run (reset + run + finalize, as bench.py's step), the time of a
read, and per round of the eager legs the load pass -- round_ms - expand_ms
against the untracked run's -- beside its algorithmic bytes (4 B per arc of
column ids, 4 B per arc of gathers, ~30 B of vertex words per vertex) and its
gather rate.  Asserts sum(sent) == sum of the rounds' sends, and for c4 that
the lazy and eager totals are equal.
usage: load_cost.py [--workload c4|c5] [--log2n N] [--steps 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_args(workload, log2n):
    import bench
    argv = ["bench.py", "--gpus", "1", "--workload", workload]
    if log2n:
        argv += ["--log2n", str(log2n)]
    old, sys.argv = sys.argv, argv
    try:
        return bench, bench.parse()
    finally:
        sys.argv = old


def engine(pkg, bench, args, track, eager=False):
    if eager:   # read at gp_create
        os.environ["GP_LOAD_EAGER"] = "1"
    else:
        os.environ.pop("GP_LOAD_EAGER", None)
    eng = pkg.GossipEngine(0, **bench.engine_config(args))
    os.environ.pop("GP_LOAD_EAGER", None)
    eng.build_chung_lu(1 << args.log2n, args.dbar, args.gamma, args.seed)
    origin = pkg.overlay.random_origins(1 << args.log2n, args.messages, seed=args.seed)
    origin = origin[eng.spread_order(origin, hops=args.spread_hops)]
    eng.set_messages(origin)
    eng.track_load(track)
    eng.reset()
    return eng


def step(eng):
    eng.synchronize()
    t0 = time.perf_counter()
    eng.reset()
    st = eng.run()
    eng.finalize()
    eng.synchronize()
    return (time.perf_counter() - t0) * 1e3, st


def read(eng):
    eng.synchronize()
    t0 = time.perf_counter()
    sent, recv = eng.load_sent(), eng.load_recv()
    return (time.perf_counter() - t0) * 1e3, sent, recv


def span(x):
    return f"{min(x):.2f} - {max(x):.2f} (median {np.median(x):.2f})"


def pass_table(say, name, st_on, st_off, n, nnz):
    """the eager pass per round: (round_ms - expand_ms) tracked less untracked"""
    nbytes = 8 * nnz + 30 * n
    say(f"{name}: load pass per round = (round_ms - expand_ms) less the untracked run's; "
        f"algorithmic bytes {nbytes / 1e6:.1f} MB (8 B x {nnz} arcs + 30 B x {n} vertices)")
    say("round     active   pass ms   GB/s   gathers G/s   round_ms (tracked)")
    tot = 0.0
    for a, b in zip(st_on, st_off):
        ms = (a["round_ms"] - a["expand_ms"]) - (b["round_ms"] - b["expand_ms"])
        tot += ms
        say(f"{a['round']:5d} {a['active']:10d} {ms:9.3f} {nbytes / max(ms, 1e-6) / 1e6:6.0f} "
            f"{nnz / max(ms, 1e-6) / 1e6:10.2f} {a['round_ms']:12.3f}")
    say(f"{name}: the passes of a run sum to {tot:.2f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("c4", "c5"), default="c4")
    ap.add_argument("--log2n", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import _gossip_pkg
    pkg = _gossip_pkg.load()
    bench, args = bench_args(a.workload, a.log2n)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{a.workload.upper()} 2^{args.log2n} x {args.messages}, bench.py's configuration, {a.steps} runs per leg")
    if a.workload == "c4":
        legs = {"untracked": engine(pkg, bench, args, False), "lazy": engine(pkg, bench, args, True),
                "eager": engine(pkg, bench, args, True, eager=True)}
        n, nnz = legs["lazy"].info()[:2]
        for e in legs.values():
            step(e)   # warm-up
        ms = {k: [] for k in legs}
        last = {}
        for _ in range(a.steps):   # alternating on the same box
            for k, e in legs.items():
                t, last[k] = step(e)
                ms[k].append(t)
        for k in legs:
            say(f"{k:9s}: ms per run {span(ms[k])}; sum of round_ms {sum(s['round_ms'] for s in last[k]):.2f}")
        t_lazy, sent, recv = read(legs["lazy"])
        t_eager, sent_e, recv_e = read(legs["eager"])
        sends = sum(s["sends"] for s in last["lazy"])
        assert int(sent.sum()) == sends == int(recv.sum()), "sent does not sum to the rounds' sends"
        assert np.array_equal(sent, sent_e) and np.array_equal(recv, recv_e), "lazy and eager totals differ"
        say(f"read of both arrays: lazy {t_lazy:.2f} ms (two passes over the in-CSR + 2 x {8 * n / 1e6:.0f} MB to the "
            f"host), eager {t_eager:.2f} ms (the copies alone); sum sent = sum recv = {sends}")
        deg = legs["lazy"].degrees()
        say(f"recv: top 1 % of the peers take {pkg.load.concentration(recv)['top_share']:.3f} of the arrivals, max / mean "
            f"{pkg.load.concentration(recv)['max_over_mean']:.0f}; max in-degree {int(deg.max())}")
        pass_table(say, "C4 eager", last["eager"], last["untracked"], n, nnz)
        for e in legs.values():
            e.close()
    else:
        ms = {"untracked": [], "tracked": []}
        last = {}
        for rep in range(2):   # alternating, one context at a time
            for k in ("untracked", "tracked"):
                with engine(pkg, bench, args, k == "tracked") as e:
                    n, nnz = e.info()[:2]
                    step(e)
                    for _ in range(max(1, a.steps // 2)):
                        t, last[k] = step(e)
                        ms[k].append(t)
                    if k == "tracked":
                        t_read, sent, recv = read(e)
        for k in ms:
            say(f"{k:9s}: ms per run {span(ms[k])}; sum of round_ms {sum(s['round_ms'] for s in last[k]):.2f}")
        sends = sum(s["sends"] for s in last["tracked"])
        assert int(sent.sum()) == sends and int(recv.sum()) <= sends
        say(f"read of both arrays {t_read:.2f} ms; sum sent {sends} = the rounds' sends, sum recv {int(recv.sum())}")
        pass_table(say, "C5", last["tracked"], last["untracked"], n, nnz)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
