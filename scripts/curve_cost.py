#!/usr/bin/env python3
"""What the spread curve costs at C4 (csrc/curve.hip).

Runs bench.py's C4 configuration (engine_config, spread message order) on two
contexts of one process, tracking off and on, alternating whole runs on the
same box, and prints:
  - ms per run (reset + run + finalize, as bench.py's step) off and on, and
    the sum of round_ms;
  - for the tracked run the three sums against the run's own counters and
    coverage (asserted): row 0 = injected, row r = new_bits of round r - 1,
    column totals = coverage;
  - per round, from a child process with GP_CURVE_YARDSTICK=1: k_curve's time
    beside the per-bit k_bitsum<W, true, false> over the same guarded frontier
    rows, and k_curve's GB/s on the bytes it reads (8W per receiver + the 4-B
    guard of every vertex).
usage: curve_cost.py [--log2n 24] [--steps 5] [--out FILE]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def engine(pkg, bench, args, track):
    eng = pkg.GossipEngine(0, **bench.engine_config(args))
    eng.build_chung_lu(1 << args.log2n, args.dbar, args.gamma, args.seed)
    origin = pkg.overlay.random_origins(1 << args.log2n, args.messages, seed=args.seed)
    origin = origin[eng.spread_order(origin, hops=args.spread_hops)]
    eng.set_messages(origin)
    eng.track_curve(track)
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


def check_sums(eng, st):
    curve = eng.curve()
    assert curve.shape == (len(st) + 1, eng.m)
    assert int(curve[0].sum()) == st[0]["injected"]
    for r in range(1, len(st) + 1):
        assert int(curve[r].sum()) == st[r - 1]["new_bits"], r
    assert np.array_equal(curve.sum(axis=0), eng.coverage())
    return curve


def bench_args(log2n):
    import bench
    argv, sys.argv = sys.argv, ["bench.py", "--gpus", "1", "--log2n", str(log2n)]
    try:
        return bench, bench.parse()
    finally:
        sys.argv = argv


def yardstick_child(log2n):
    """one tracked run with the library's yardstick on; the rounds' counters go to stdout"""
    import _gossip_pkg
    pkg = _gossip_pkg.load()
    bench, args = bench_args(log2n)
    with engine(pkg, bench, args, True) as eng:
        step(eng)   # warm
        sys.stderr.write("gp_curve_yardstick begin\n")
        sys.stderr.flush()
        _, st = step(eng)
        check_sums(eng, st)
        print(json.dumps(dict(n=eng.n, words=eng.words, rounds=[dict(round=s["round"], receivers=s["receivers"],
                                                                     new_bits=s["new_bits"]) for s in st])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--yardstick-child", action="store_true")
    a = ap.parse_args()
    if a.yardstick_child:
        return yardstick_child(a.log2n)
    import _gossip_pkg
    pkg = _gossip_pkg.load()
    bench, args = bench_args(a.log2n)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    off, on = engine(pkg, bench, args, False), engine(pkg, bench, args, True)
    step(off), step(on)   # warm-up
    ms = {"off": [], "on": []}
    rms = {"off": [], "on": []}
    for _ in range(a.steps):   # alternating on the same box
        for name, eng in (("off", off), ("on", on)):
            t, st = step(eng)
            ms[name].append(t)
            rms[name].append(sum(s["round_ms"] for s in st))
    curve = check_sums(on, st)
    say(f"C4 2^{a.log2n} x {args.messages}, bench.py's configuration, {a.steps} alternating runs per leg")
    for name in ("off", "on"):
        say(f"tracking {name:3s}: ms per run {min(ms[name]):.2f} - {max(ms[name]):.2f} (median {np.median(ms[name]):.2f}); "
            f"sum of round_ms {min(rms[name]):.2f} - {max(rms[name]):.2f}")
    say(f"three sums against the run's own counters and coverage: ok ({curve.shape[0]} rows, "
        f"{int(curve.sum())} first receipts)")
    cum = pkg.spread.cumulative(curve)
    t = pkg.spread.rounds_to_reach(curve, None, 0.99, of=on.n)
    say(f"rounds to reach 99 % of the peers: min {t[t >= 0].min()} max {t.max()} (never: {(t < 0).sum()}); "
        f"coverage after each round, slowest message: {cum[:, -1].tolist()}")
    off.close()
    on.close()
    env = dict(os.environ, GP_CURVE_YARDSTICK="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--yardstick-child", "--log2n", str(a.log2n)],
                       env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("yardstick child failed")
    info = json.loads(p.stdout.strip().splitlines()[-1])
    timed = p.stderr.split("gp_curve_yardstick begin")[-1]
    rows = re.findall(r"round=(\d+) words=(\d+) k_curve_ms=([\d.]+) k_bitsum_ms=([\d.]+) equal=(\d)", timed)
    assert len(rows) == len(info["rounds"]) and all(r[4] == "1" for r in rows), "k_curve and k_bitsum disagree"
    say("round  receivers   new_bits      k_curve ms  k_bitsum ms  ratio   k_curve GB/s (rows + guards)")
    for (r, w, tc, tb, _), s in zip(rows, info["rounds"]):
        nbytes = s["receivers"] * 8 * int(w) + info["n"] * 4
        tc, tb = float(tc), float(tb)
        say(f"{int(r):5d} {s['receivers']:10d} {s['new_bits']:12d} {tc:11.4f} {tb:12.4f} {tb / max(tc, 1e-9):6.2f} "
            f"{nbytes / max(tc, 1e-9) / 1e6:10.1f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
