#!/usr/bin/env python3
"""What the per-peer fresh-delivery record costs (csrc/fresh.hip).

Runs bench.py's configuration (engine_config, spread message order) on the
same box, alternating whole runs:
  c4   untracked, tracked (one gather, the senders' side by atomics: the
       default form) and tracked with GP_FRESH_GATHER=1 (one gather per role,
       no per-arc atomics), three contexts of one process;
  c5   untracked and tracked, one context at a time (two 2^26 x 4096 contexts
       with frontier rows do not fit beside each other).
Prints ms per run (reset + run + finalize, as bench.py's step), the time of a
read, and per round of the tracked legs the pass -- round_ms - expand_ms
against the untracked run's -- beside the same round's kernel_ms and
expand_ms, the yardstick of what a gather over those arcs costs.  Asserts
sum(fresh_sent) == sum(fresh_recv) >= the run's new_bits, and for c4 that both
forms give the same arrays.
usage: fresh_cost.py [--workload c4|c5] [--log2n N] [--steps 5] [--out FILE]
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


def engine(pkg, bench, args, track, gather=False):
    if gather:   # read at gp_create
        os.environ["GP_FRESH_GATHER"] = "1"
    else:
        os.environ.pop("GP_FRESH_GATHER", None)
    eng = pkg.GossipEngine(0, **bench.engine_config(args))
    os.environ.pop("GP_FRESH_GATHER", None)
    eng.build_chung_lu(1 << args.log2n, args.dbar, args.gamma, args.seed)
    origin = pkg.overlay.random_origins(1 << args.log2n, args.messages, seed=args.seed)
    origin = origin[eng.spread_order(origin, hops=args.spread_hops)]
    eng.set_messages(origin)
    eng.track_fresh(track)
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
    sent, recv = eng.fresh_sent(), eng.fresh_recv()
    return (time.perf_counter() - t0) * 1e3, sent, recv


def span(x):
    return f"{min(x):.2f} - {max(x):.2f} (median {np.median(x):.2f})"


def pass_table(say, name, st_on, st_off):
    """the pass per round: (round_ms - expand_ms) tracked less untracked"""
    say(f"{name}: fresh pass per round = (round_ms - expand_ms) less the untracked run's, beside the round's own pull")
    say("round     active  receivers   pass ms   kernel_ms  expand_ms   pass / expand")
    tot = exp = 0.0
    for a, b in zip(st_on, st_off):
        ms = (a["round_ms"] - a["expand_ms"]) - (b["round_ms"] - b["expand_ms"])
        tot += ms
        exp += a["expand_ms"]
        say(f"{a['round']:5d} {a['active']:10d} {a['receivers']:10d} {ms:9.3f} {a['kernel_ms']:11.3f} "
            f"{a['expand_ms']:10.3f} {ms / max(a['expand_ms'], 1e-6):10.2f}")
    say(f"{name}: the passes of a run sum to {tot:.2f} ms, its expansions to {exp:.2f} ms")


def check(sent, recv, stats):
    new = sum(s["new_bits"] for s in stats)
    assert int(sent.sum()) == int(recv.sum()) >= new, "fresh_sent and fresh_recv do not add up"
    return int(recv.sum()), new, sum(s["sends"] for s in stats)


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
        legs = {"untracked": engine(pkg, bench, args, False), "scatter": engine(pkg, bench, args, True),
                "gather": engine(pkg, bench, args, True, gather=True)}
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
        t_read, sent, recv = read(legs["scatter"])
        _, sent_s, recv_s = read(legs["gather"])
        assert np.array_equal(sent, sent_s) and np.array_equal(recv, recv_s), "the two forms differ"
        fresh, new, sends = check(sent, recv, last["scatter"])
        say(f"read of both arrays {t_read:.2f} ms (2 x {8 * sent.size / 1e6:.0f} MB to the host); fresh deliveries {fresh}, "
            f"first receipts {new}, sends {sends}: relative message redundancy "
            f"{pkg.redundancy.relative_redundancy(np.array([sends]), new):.2f}, fresh / first receipts {fresh / max(new, 1):.3f}")
        c = pkg.redundancy.concentration(sent)
        say(f"fresh_sent: top 1 % of the peers deliver {c['top_share']:.3f} of the news, max / mean {c['max_over_mean']:.0f}")
        pass_table(say, "C4 scatter", last["scatter"], last["untracked"])
        pass_table(say, "C4 gather", last["gather"], last["untracked"])
        for e in legs.values():
            e.close()
    else:
        ms = {"untracked": [], "tracked": []}
        last = {}
        for rep in range(2):   # alternating, one context at a time
            for k in ("untracked", "tracked"):
                with engine(pkg, bench, args, k == "tracked") as e:
                    step(e)
                    for _ in range(max(1, a.steps // 2)):
                        t, last[k] = step(e)
                        ms[k].append(t)
                    if k == "tracked":
                        t_read, sent, recv = read(e)
        for k in ms:
            say(f"{k:9s}: ms per run {span(ms[k])}; sum of round_ms {sum(s['round_ms'] for s in last[k]):.2f}")
        fresh, new, sends = check(sent, recv, last["tracked"])
        say(f"read of both arrays {t_read:.2f} ms; fresh deliveries {fresh}, first receipts {new}, sends {sends}")
        pass_table(say, "C5", last["tracked"], last["untracked"])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
