#!/usr/bin/env python3
"""CPU estimate of the per-line done-neighbour rule (DESIGN.md §3.3 "Complete
lines of a top in-neighbour"): how many 128-B row lines the early-exit pull
rounds of a C4-recipe run fetch with and without it.

The CPU oracle runs the Chung-Lu recipe of C4 (d 16, gamma 2.5, seed 4, 4096
messages) at 2^LOG2N with the message table in the bench's spread order
(overlay.spread_keys, 3 hops); its first-receipt matrix gives every
Message-List at the start of every round.  For a sample of receivers the
script then walks the gather as k_expand does:
  parent: receivers still lacking messages, in-lists in gather order
          (neighbour in-degree descending, ties by id), rows in batches (6 in
          the serial loop; 2 for in-degree <= 32 once most messages are held,
          gather_pairs), a lane (16 B) loads its piece of a batch's rows while
          its two words still lack messages, a line is fetched when one of
          its 8 lanes loads; done_nb over the first two arcs once half the
          bits are held;
  rule:   the same with the lines that one of the first two gather-order
          in-neighbours of in-degree >= T held whole at the start of the round
          taken as covered before the first batch.
usage: line_done_estimate.py [--log2n 20] [--sample 12000] [--threads 8]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import _gossip_pkg  # noqa: E402
from oracle import lib as oracle_lib  # noqa: E402

M, LANES, LINES = 4096, 32, 4
HUB_THR = 4096
THRESHOLDS = (64, 256, 1024)


def lanes_any(bits):        # [.., 4096] bool -> [.., 32] lanes holding a set bit
    return bits.reshape(bits.shape[:-1] + (LANES, M // LANES)).any(-1)


def walk(want, rows, batch):
    """Lines fetched and rows gathered for one receiver: want [4096] bool, rows
    [deg, 4096] bool in gather order."""
    lines = nrows = 0
    acc = np.zeros(M, bool)
    for k0 in range(0, rows.shape[0], batch):
        live = lanes_any(want & ~acc)
        if not live.any():
            break
        nb = min(batch, rows.shape[0] - k0)
        lines += nb * int(live.reshape(LINES, 8).any(1).sum())
        nrows += nb
        keep = np.repeat(live, M // LANES)
        acc |= rows[k0:k0 + nb].any(0) & keep
    return lines, nrows, acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--sample", type=int, default=12000)
    ap.add_argument("--threads", type=int, default=8)
    a = ap.parse_args()
    pkg = _gossip_pkg.load()
    n = 1 << a.log2n
    rp, col = oracle_lib.chung_lu(n, 16.0, 2.5, 4)
    g = pkg.overlay.CSR(n, rp, col, False)
    origin = pkg.overlay.random_origins(n, M, 4)
    origin = origin[pkg.overlay.spread_order(pkg.overlay.spread_keys(rp, col, origin, 3))]
    ref = oracle_lib.run(g, origin, want_first=True, want_seen=False, want_forwards=False, nthreads=a.threads)
    first = ref["first"]
    deg = np.diff(rp)
    print(f"n=2^{a.log2n} nnz={g.nnz} rounds={ref['rounds']} max in-degree={int(deg.max())} "
          f"vertices of in-degree >= " + ", ".join(f"{t}: {int((deg >= t).sum())}" for t in THRESHOLDS))
    rng = np.random.Generator(np.random.PCG64(1))
    sample = rng.choice(n, min(a.sample, n), replace=False)
    nm = float(n) * M
    print("| round | held at start | early exit | done_nb | receivers sampled | lines, parent | "
          + " | ".join(f"T={t}: lines (saved), complete lines / receiver" for t in THRESHOLDS) + " |")
    for r in range(1, ref["rounds"]):
        held = float(sum(s["new_bits"] + s["injected"] for s in ref["stats"][:r]))
        new_prev = float(ref["stats"][r - 1]["new_bits"])
        ee = new_prev * 16.0 >= nm or held * 2.0 >= nm
        dnb = ee and held * 2.0 >= nm
        if not ee:
            continue
        tot_parent, tot_rule = 0, {t: 0 for t in THRESHOLDS}
        found = {t: 0 for t in THRESHOLDS}
        nrecv = 0
        for v in sample:
            d = int(deg[v])
            if d == 0 or d > HUB_THR:
                continue
            cm = first[v] != 255                 # final Message-List = the component's messages
            seen = first[v] <= r
            want = cm & ~seen
            if not want.any():
                continue
            nb = col[rp[v]:rp[v + 1]]
            nb = nb[np.lexsort((nb, -deg[nb]))]  # gather order
            rows = first[nb] <= r
            if dnb and (rows[:2] | ~cm).all(1).any():
                continue                         # a done in-neighbour: no gather, parent and rule alike
            nrecv += 1
            batch = 2 if (dnb and d <= 32) else 6
            lp, _, _ = walk(want, rows, batch)
            tot_parent += lp
            top = rows[:2] | ~cm
            top_lines = top.reshape(-1, LINES, M // LINES).all(2)       # [<= 2, 4] line held whole
            for t in THRESHOLDS:
                ld = (top_lines & (deg[nb[:2]] >= t)[:, None]).any(0)   # [4]
                w2 = want & ~np.repeat(ld, M // LINES)
                found[t] += int((ld & want.reshape(LINES, -1).any(1)).sum())
                lr, _, _ = walk(w2, rows, batch)
                tot_rule[t] += lr
        cells = " | ".join(
            f"{tot_rule[t]} ({100.0 * (tot_parent - tot_rule[t]) / max(tot_parent, 1):.0f} %), "
            f"{found[t] / max(nrecv, 1):.2f}" for t in THRESHOLDS)
        print(f"| {r} | {100.0 * held / nm:.0f} % | {'yes' if ee else 'no'} | {'yes' if dnb else 'no'} | {nrecv} | "
              f"{tot_parent} | {cells} |", flush=True)


if __name__ == "__main__":
    main()
