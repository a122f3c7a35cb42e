#!/usr/bin/env python3
"""What the per-link fresh-delivery record costs (csrc/link.hip).

Runs bench.py's configuration (engine_config, spread message order) on the
same box, alternating whole runs:
  c4   untracked, tracked per peer (gp_track_fresh, k_fresh's scatter pass) and
       tracked per link (gp_track_link_fresh, k_link), three contexts of one
       process;
  c5   the same three, one context at a time (two 2^26 x 4096 contexts with
       frontier rows do not fit beside each other).
Prints ms per run (reset + run + finalize, as bench.py's step) and, per round,
the two passes -- round_ms - expand_ms against the untracked run's -- side by
side with their ratio; then the cost of a full read of the u16[nnz], of
gp_read_link_hist, and what the histogram says: the idle-arc share and the
fewest arcs that carry half of the news.  Asserts that the per-link record
folds into the per-peer totals of the other leg (c4), that its sum is theirs,
and that the device histogram is the bincount of the array.
usage: link_cost.py [--workload c4|c5] [--log2n N] [--steps 5] [--out FILE]
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


def engine(pkg, bench, args, track):
    eng = pkg.GossipEngine(0, **bench.engine_config(args))
    eng.build_chung_lu(1 << args.log2n, args.dbar, args.gamma, args.seed)
    origin = pkg.overlay.random_origins(1 << args.log2n, args.messages, seed=args.seed)
    origin = origin[eng.spread_order(origin, hops=args.spread_hops)]
    eng.set_messages(origin)
    if track == "fresh":
        eng.track_fresh()
    elif track == "link":
        eng.track_link_fresh()
    eng.reset()
    return eng


def timed(eng, fn):
    eng.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def pass_table(say, name, st_fresh, st_link, st_off):
    """the passes per round: (round_ms - expand_ms) tracked less untracked"""
    say(f"{name}: pass per round = (round_ms - expand_ms) less the untracked run's: k_fresh (per peer, scatter) "
        "beside k_link (per link)")
    say("round     active  receivers  k_fresh ms  k_link ms  expand_ms  link / fresh")
    tf = tl = 0.0
    for f, l, u in zip(st_fresh, st_link, st_off):
        base = u["round_ms"] - u["expand_ms"]
        pf = (f["round_ms"] - f["expand_ms"]) - base
        pl = (l["round_ms"] - l["expand_ms"]) - base
        tf += pf
        tl += pl
        say(f"{l['round']:5d} {l['active']:10d} {l['receivers']:10d} {pf:11.3f} {pl:10.3f} {l['expand_ms']:10.3f} "
            f"{pl / max(pf, 1e-6):10.2f}")
    say(f"{name}: the passes of a run sum to {tf:.2f} ms (k_fresh) and {tl:.2f} ms (k_link), ratio {tl / max(tf, 1e-6):.2f}")


def report(say, pkg, eng, stats, sent=None, recv=None):
    t_read, lf = timed(eng, eng.link_fresh)
    t_hist, h = timed(eng, eng.link_hist)
    t_hist2, _ = timed(eng, eng.link_hist)
    assert np.array_equal(h, pkg.links.hist(lf)), "the device histogram is not the array's"
    total = int(lf.sum(dtype=np.int64))
    new = sum(s["new_bits"] for s in stats)
    assert total >= new
    if sent is not None:
        fs, fr = pkg.links.fold_peers(eng.graph(), lf)
        assert np.array_equal(fs, sent.astype(np.int64)) and np.array_equal(fr, recv.astype(np.int64)), \
            "the per-link record does not fold into the per-peer totals"
    say(f"read of the record {t_read:.2f} ms ({2 * lf.size / 1e6:.0f} MB to the host); gp_read_link_hist "
        f"{t_hist:.2f} ms, again {t_hist2:.2f} ms (33 KB to the host)")
    arcs, least = pkg.links.hist_backbone(h, 0.5)
    say(f"arcs {lf.size}, fresh deliveries {total}, first receipts {new}; idle arcs {int(h[0])} "
        f"({int(h[0]) / max(lf.size, 1):.4f} of all); max count {int(np.nonzero(h)[0].max())}; half of the news over "
        f"{arcs} arcs ({arcs / max(lf.size, 1):.4f} of all), each carrying >= {least}")
    for share in (0.9, 0.99):
        k, c = pkg.links.hist_backbone(h, share)
        say(f"  {share:.2f} of the news over {k} arcs ({k / max(lf.size, 1):.4f}), each >= {c}")


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

    names = ("untracked", "fresh", "link")
    say(f"{a.workload.upper()} 2^{args.log2n} x {args.messages}, bench.py's configuration, {a.steps} runs per leg")
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
        for k in names:
            say(f"{k:9s}: ms per run {span(ms[k])}; sum of round_ms {sum(s['round_ms'] for s in last[k]):.2f}")
        pass_table(say, "C4", last["fresh"], last["link"], last["untracked"])
        report(say, pkg, legs["link"], last["link"], legs["fresh"].fresh_sent(), legs["fresh"].fresh_recv())
        for e in legs.values():
            e.close()
    else:
        for k in names:   # one context at a time
            with engine(pkg, bench, args, k) as e:
                step(e)
                for _ in range(max(1, a.steps // 2)):
                    t, last[k] = step(e)
                    ms[k].append(t)
                say(f"{k:9s}: ms per run {span(ms[k])}; sum of round_ms {sum(s['round_ms'] for s in last[k]):.2f}")
                flush()
                if k == "link":
                    pass_table(say, "C5", last["fresh"], last["link"], last["untracked"])
                    report(say, pkg, e, last["link"])
    flush()


if __name__ == "__main__":
    main()
