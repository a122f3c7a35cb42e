#!/usr/bin/env python3
"""What the fresh-delivery curve costs (csrc/fresh_curve.hip).

Runs bench.py's configuration (engine_config, spread message order) on the
same box, alternating whole runs:
  c4   untracked, tracked per peer (gp_track_fresh, k_fresh's scatter pass:
       the yardstick, the same row pairs with per-arc atomics) and tracked per
       message (gp_track_fresh_curve, k_fresh_curve), three contexts of one
       process;
  c5   the same three, one context at a time (two 2^26 x 4096 contexts with
       frontier rows do not fit beside each other).
Prints ms per run (reset + run + finalize, as bench.py's step), the time of a
read, and per round of the tracked legs the pass -- round_ms - expand_ms
against the untracked run's -- of both records beside the same round's
kernel_ms and expand_ms.  Asserts that the record's row sums are the growth of
sum(fresh_recv) -- the two tracked legs are the same run -- and that its
columns lie between coverage - 1 and forwards.

--parent-tree DIR (a checkout of the parent commit with its library built):
untracked against the parent, `bench.py --gpus 1 --steps S --warmup 1
--dump-outputs` of both trees alternating as child processes, --pairs times:
the job record of the bench line and every dumped file must be identical, and
the ms per step of both are printed beside each other -- the box's own
run-to-run spread is the spread within one tree's lines.
usage: fresh_curve_cost.py [--workload c4|c5] [--log2n N] [--steps 5] [--out FILE]
                           [--parent-tree DIR [--pairs 3]]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
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


def engine(pkg, bench, args, track):
    eng = pkg.GossipEngine(0, **bench.engine_config(args))
    eng.build_chung_lu(1 << args.log2n, args.dbar, args.gamma, args.seed)
    origin = pkg.overlay.random_origins(1 << args.log2n, args.messages, seed=args.seed)
    origin = origin[eng.spread_order(origin, hops=args.spread_hops)]
    eng.set_messages(origin)
    if track == "fresh":
        eng.track_fresh()
    elif track == "fresh_curve":
        eng.track_fresh_curve()
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


def span(x):
    return f"{min(x):.2f} - {max(x):.2f} (median {np.median(x):.2f})"


def pass_table(say, name, st_peer, st_msg, st_off):
    """the passes per round: (round_ms - expand_ms) tracked less untracked"""
    say(f"{name}: pass per round = (round_ms - expand_ms) less the untracked run's; k_fresh (per peer, scatter) "
        "beside k_fresh_curve (per message), and the round's own pull")
    say("round     active  receivers  k_fresh ms  k_fresh_curve ms  kernel_ms  expand_ms  curve / fresh")
    tp = tm = 0.0
    for a, b, c in zip(st_peer, st_msg, st_off):
        base = c["round_ms"] - c["expand_ms"]
        p = (a["round_ms"] - a["expand_ms"]) - base
        m = (b["round_ms"] - b["expand_ms"]) - base
        tp += p
        tm += m
        say(f"{b['round']:5d} {b['active']:10d} {b['receivers']:10d} {p:11.3f} {m:17.3f} {b['kernel_ms']:10.3f} "
            f"{b['expand_ms']:10.3f} {m / max(p, 1e-6):14.2f}")
    say(f"{name}: the passes of a run sum to {tp:.2f} ms (k_fresh) and {tm:.2f} ms (k_fresh_curve)")


def check(fc, recv_total, cov, fwd, stats):
    fc = fc.astype(np.int64)
    assert not fc[0].any() and int(fc.sum()) == recv_total, "the record does not sum to sum(fresh_recv)"
    assert int(fc.sum()) >= sum(s["new_bits"] for s in stats)
    col = fc.sum(axis=0)
    assert (col >= np.maximum(cov.astype(np.int64) - 1, 0)).all(), "a first receipt without a deliverer"
    if fwd is not None:
        assert (col <= fwd.astype(np.int64)).all(), "more deliveries than sends"
    return col


def bench_line(tree, workload, log2n, steps, dump):
    cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--workload", workload, "--dump-outputs", dump]
    if log2n:
        cmd += ["--log2n", str(log2n)]
    out = subprocess.run(cmd, cwd=tree, check=True, stdout=subprocess.PIPE, text=True).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def against_parent(say, a, parent):
    say(f"untracked against the parent tree: bench.py --gpus 1 --steps {a.steps} --warmup 1, child processes "
        f"alternating, {a.pairs} pairs")
    ms = {"parent": [], "this": []}
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(a.pairs):
            dumps = {}
            for name, tree in (("parent", parent), ("this", ROOT)):
                dumps[name] = os.path.join(tmp, f"{name}{i}")
                line = bench_line(tree, a.workload, a.log2n, a.steps, dumps[name])
                ms[name].append(line["ms_per_step"])
                dumps[name + "_job"] = line["config"]["job"]
            assert dumps["parent_job"] == dumps["this_job"], "the job records differ"
            files = sorted(os.listdir(dumps["parent"]))
            assert files and files == sorted(os.listdir(dumps["this"])), "different dumped files"
            for f in files:
                x, y = np.load(os.path.join(dumps["parent"], f)), np.load(os.path.join(dumps["this"], f))
                assert x.shape == y.shape and np.array_equal(x, y), f"{f} differs"
        say(f"  job record and {len(files)} dumped files identical in every pair")
    for name in ms:
        say(f"  {name:6s}: ms per step " + " / ".join(f"{x:.2f}" for x in ms[name]) + f"; {span(ms[name])}")


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

    def save():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if a.parent_tree:   # (before this process opens the GPU: the children time alone)
        against_parent(say, a, os.path.abspath(a.parent_tree))
        save()
    import _gossip_pkg
    pkg = _gossip_pkg.load()
    bench, args = bench_args(a.workload, a.log2n)
    say(f"{a.workload.upper()} 2^{args.log2n} x {args.messages}, bench.py's configuration, {a.steps} runs per leg")
    names = ("untracked", "fresh", "fresh_curve")
    ms = {k: [] for k in names}
    last = {}
    if a.workload == "c4":
        legs = {k: engine(pkg, bench, args, k) for k in names}
        for e in legs.values():
            step(e)   # warm-up
        for _ in range(a.steps):   # alternating on the same box
            for k, e in legs.items():
                t, last[k] = step(e)
                ms[k].append(t)
        recv_total = int(legs["fresh"].fresh_recv().astype(np.int64).sum())
        e = legs["fresh_curve"]
        e.synchronize()
        t0 = time.perf_counter()
        fc = e.fresh_curve()
        t_read = (time.perf_counter() - t0) * 1e3
        cov = e.coverage()
        for e in legs.values():
            e.close()
    else:
        for rep in range(2):   # alternating, one context at a time
            for k in names:
                with engine(pkg, bench, args, k) as e:
                    step(e)
                    for _ in range(max(1, a.steps // 2)):
                        t, last[k] = step(e)
                        ms[k].append(t)
                    if k == "fresh":
                        recv_total = int(e.fresh_recv().astype(np.int64).sum())
                    if k == "fresh_curve":
                        e.synchronize()
                        t0 = time.perf_counter()
                        fc = e.fresh_curve()
                        t_read = (time.perf_counter() - t0) * 1e3
                        cov = e.coverage()
    for k in names:
        say(f"{k:11s}: ms per run {span(ms[k])}; sum of round_ms {sum(s['round_ms'] for s in last[k]):.2f}, "
            f"of expand_ms {sum(s['expand_ms'] for s in last[k]):.2f}")
    col = check(fc, recv_total, cov, None, last["fresh_curve"])
    red = pkg.redundancy
    per = red.deliverers_per_receipt(fc, cov)
    say(f"read of the record {t_read:.2f} ms ({fc.shape[0]} rows x {fc.shape[1]} u64); deliveries {int(col.sum())} = "
        f"sum fresh_recv, first receipts {sum(s['new_bits'] for s in last['fresh_curve'])}; deliverers per first "
        f"receipt over the messages: min {per[per > 0].min():.2f}, median {np.median(per[per > 0]):.2f}, "
        f"max {per.max():.2f}")
    rows = fc.astype(np.int64).sum(axis=1)
    say("deliveries by receipt round: " + " ".join(str(int(x)) for x in rows))
    pass_table(say, a.workload.upper(), last["fresh"], last["fresh_curve"], last["untracked"])
    save()


if __name__ == "__main__":
    main()
