#!/usr/bin/env python3
"""What watching peers costs (csrc/watch.hip).

Runs bench.py's configuration (engine_config, spread message order) on one box,
alternating whole runs of the contexts of one process: unwatched, and three
watch lists --
  rand64    64 random peers
  hubs64    the 64 peers of highest in-degree
  rand4096  4,096 random peers
Prints each list's A (watched arcs) and the record's bytes, ms per run (reset +
run + finalize, as bench.py's step) and, per round, each list's pass --
round_ms - expand_ms against the unwatched run's -- beside the round's
expand_ms of that leg.  Then the cost of the reads, and the per-peer identities
the log must satisfy on the engine's own counters (every watched peer's held
messages against seenpop, every arrival no earlier than the first receipt).
--parent-tree DIR first times bench.py of DIR against this tree's, no list set,
in alternating child processes (job record and dumped outputs compared).
usage: watch_cost.py [--workload c4|c5] [--log2n N] [--steps 5] [--out FILE] [--parent-tree DIR --pairs 3]
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


def engine(pkg, bench, args, verts):
    eng = pkg.GossipEngine(0, **bench.engine_config(args))
    eng.build_chung_lu(1 << args.log2n, args.dbar, args.gamma, args.seed)
    origin = pkg.overlay.random_origins(1 << args.log2n, args.messages, seed=args.seed)
    origin = origin[eng.spread_order(origin, hops=args.spread_hops)]
    eng.set_messages(origin)
    if verts is not None:
        eng.watch(verts(eng), max_bytes=1 << 36)
    eng.reset()
    return eng


def lists(seed):
    def rand(k):
        return lambda eng: np.random.default_rng(seed).choice(eng.n, k, replace=False)

    def hubs(k):
        return lambda eng: np.argsort(-eng.degrees().astype(np.int64), kind="stable")[:k]
    return {"unwatched": None, "rand64": rand(64), "hubs64": hubs(64), "rand4096": rand(4096)}


def timed(eng, fn):
    eng.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


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
    legs = lists(args.seed)
    engs = {k: engine(pkg, bench, args, v) for k, v in legs.items()}
    watched = [k for k in legs if k != "unwatched"]
    for k in watched:
        peers, arcs, nbytes = engs[k].watch_info()
        say(f"{k:9s}: K = {peers}, A = {arcs} watched arcs, record {nbytes / 2**20:.1f} MiB "
            f"(index arrays {8 * arcs / 2**20:.2f} MiB)")
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
    per = {k: [(x["round_ms"] - x["expand_ms"]) - (y["round_ms"] - y["expand_ms"])
               for x, y in zip(last[k], last["unwatched"])] for k in watched}
    say("pass per round = (round_ms - expand_ms) less the unwatched run's, ms, beside that leg's expand_ms")
    say("round     active  receivers " + " ".join(f"{k + ' pass':>14s} {'expand':>8s}" for k in watched) +
        "   expand unwatched")
    for i, s in enumerate(last["unwatched"]):
        say(f"{s['round']:5d} {s['active']:10d} {s['receivers']:10d} " +
            " ".join(f"{per[k][i]:14.3f} {last[k][i]['expand_ms']:8.3f}" for k in watched) + f" {s['expand_ms']:18.3f}")
    for k in watched:
        worst = max(range(len(per[k])), key=lambda i: per[k][i])
        say(f"{k:9s}: the passes of a run sum to {sum(per[k]):.2f} ms; the largest, round {worst}: {per[k][worst]:.3f} ms "
            f"against expand_ms {last[k][worst]['expand_ms']:.3f}")
    flush()
    for k in watched:
        eng = engs[k]
        t_first, first = timed(eng, eng.watch_first)
        t_arr, arr = timed(eng, eng.watch_arrival)
        t_peer, (f0, a0) = timed(eng, lambda: eng.watch_peer(0))
        ptr, sp = eng.watch_ptr(), eng.seenpop()
        verts = legs[k](eng)
        assert np.array_equal((first != 255).sum(axis=1), sp[verts]), "held messages differ from seenpop"
        slot = np.repeat(np.arange(len(verts)), np.diff(ptr))
        got = arr != 255
        assert (first[slot][got] <= arr[got]).all(), "an arrival before the first receipt"
        assert np.array_equal(f0, first[0]) and np.array_equal(a0, arr[ptr[0]:ptr[1]])
        fresh = int((got & (arr == first[slot])).sum())
        say(f"{k:9s}: read of watch_first {t_first:.2f} ms ({first.nbytes / 2**20:.1f} MiB), watch_arrival {t_arr:.2f} ms "
            f"({arr.nbytes / 2**20:.1f} MiB), one peer (in-degree {int(ptr[1] - ptr[0])}) {t_peer:.2f} ms; "
            f"{int(got.sum())} lines, {fresh} fresh, {100.0 * got.mean():.1f} % of the cells written")
    for e in engs.values():
        e.close()
    flush()


if __name__ == "__main__":
    main()
