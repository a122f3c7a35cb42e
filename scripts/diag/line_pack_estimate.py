#!/usr/bin/env python3
"""CPU estimate of the packed row gather (DESIGN.md §3.3 "The packed gather"):
how many dependent gather round trips and how many 128-B row lines the
early-exit pull rounds of a C4-recipe run take with the row layout (32 lanes
per row to the end) and with the lanes dealt out over the live lines.

Same oracle run, recipe, seed and walk as line_done_estimate.py: the CPU oracle
runs the Chung-Lu recipe of C4 (d 16, gamma 2.5, seed 4, 4096 messages) at
2^LOG2N with the message table in the bench's spread order; its first-receipt
matrix gives every Message-List at the start of every round.  For a sample of
receivers the script walks the gather as k_expand does: in-lists in gather
order, 64 arcs per pass, done_nb over the first two arcs once half the bits
are held, the per-line done-neighbour rule (candidates of in-degree >= 64) in
the early-exit rounds before that, as by default.
  now:    batches of RIF x 2 rows in the serial loop (RIF 3), of RIF rows per
          receiver in gather_pairs (in-degree <= 32 once half the bits are
          held, RIF 2); a line of a batch's rows is fetched while one of its
          8 lanes still misses messages in its two words;
  packed: before every batch the live lines are counted: with one a batch
          holds 4x the rows, with two 2x, and only those lines are fetched.
A trip is one batch: the loads of a batch are in flight together, the next
batch waits for them.
usage: line_pack_estimate.py [--log2n 20] [--sample 4000] [--threads 8]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import _gossip_pkg  # noqa: E402
from oracle import lib as oracle_lib  # noqa: E402

M, LANES, LINES = 4096, 32, 4
HUB_THR, LD_MIN_DEG, PASS = 4096, 64, 64
SERIAL_RIF, PAIR_RIF = 3, 2


def live_lanes(bits):       # [4096] bool -> [32] lanes whose two words hold a set bit
    return bits.reshape(LANES, M // LANES).any(-1)


def walk(want, rows, acc, base, rif, packed, hist):
    """One receiver: base rows per wave-instruction (2 serial, 1 per half in
    pairs), rif instructions per batch.  Returns (trips, lines)."""
    trips = lines = 0
    acc = acc.copy()
    for p0 in range(0, rows.shape[0], PASS):
        p1 = min(p0 + PASS, rows.shape[0])
        k0 = p0
        while k0 < p1:
            live = live_lanes(want & ~acc)
            nl = int(live.reshape(LINES, 8).any(1).sum())
            if nl == 0:
                return trips, lines
            if hist is not None:
                hist[nl - 1] += 1
            mult = (4 if nl == 1 else 2 if nl == 2 else 1) if packed else 1
            nb = min(rif * base * mult, p1 - k0)
            trips += 1
            lines += nb * nl
            acc |= rows[k0:k0 + nb].any(0) & np.repeat(live, M // LANES)
            k0 += nb
    return trips, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--sample", type=int, default=4000)
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
    print(f"n=2^{a.log2n} nnz={g.nnz} rounds={ref['rounds']} max in-degree={int(deg.max())}")
    rng = np.random.Generator(np.random.PCG64(1))
    sample = rng.choice(n, min(a.sample, n), replace=False)
    nm = float(n) * M
    sweep = [("serial", r) for r in (1, 2, 3)] + [("pairs", r) for r in (1, 2)]
    print("| round | receivers (serial / pairs) | trips, now | lines, now | "
          + " | ".join(f"{k} RIF {r}: trips, lines" for k, r in sweep)
          + " | live lines per batch, now (1 / 2 / 3 / 4) | at the first batch | at the second |")
    for r in range(1, ref["rounds"]):
        held = float(sum(s["new_bits"] + s["injected"] for s in ref["stats"][:r]))
        ee = float(ref["stats"][r - 1]["new_bits"]) * 16.0 >= nm or held * 2.0 >= nm
        dnb = ee and held * 2.0 >= nm
        if not ee:
            continue
        now = {"serial": [0, 0], "pairs": [0, 0]}
        pk = {s: [0, 0] for s in sweep}
        nrecv = {"serial": 0, "pairs": 0}
        hist, h1, h2 = [0] * 4, [0] * 4, [0] * 4
        for v in sample:
            d = int(deg[v])
            if d == 0 or d > HUB_THR:
                continue
            cm = first[v] != 255
            want = cm & ~(first[v] <= r)
            if not want.any():
                continue
            nb = col[rp[v]:rp[v + 1]]
            nb = nb[np.lexsort((nb, -deg[nb]))]
            rows = first[nb] <= r
            top = rows[:2] | ~cm
            if dnb and top.all(1).any():
                continue                       # a done in-neighbour: no gather
            acc = np.zeros(M, bool)
            if not dnb:                        # the per-line rule (default gate: before the done-neighbour rounds)
                ld = (top.reshape(-1, LINES, M // LINES).all(2) & (deg[nb[:2]] >= LD_MIN_DEG)[:, None]).any(0)
                acc = want & np.repeat(ld, M // LINES)
                if not (want & ~acc).any():
                    continue
            kind = "pairs" if (dnb and d <= 32) else "serial"
            base, rif = (1, PAIR_RIF) if kind == "pairs" else (2, SERIAL_RIF)
            nrecv[kind] += 1
            hb = [0] * 4
            t, l = walk(want, rows, acc, base, rif, False, hb)
            now[kind][0] += t
            now[kind][1] += l
            for q in range(4):
                hist[q] += hb[q]
            # live lines before the first and the second batch
            f = int(live_lanes(want & ~acc).reshape(LINES, 8).any(1).sum())
            h1[f - 1] += 1
            a2 = acc | (rows[:rif * base].any(0) & np.repeat(live_lanes(want & ~acc), M // LANES))
            s2 = int(live_lanes(want & ~a2).reshape(LINES, 8).any(1).sum())
            if s2 and d > rif * base:
                h2[s2 - 1] += 1
            for s in sweep:
                if s[0] == kind:
                    t, l = walk(want, rows, acc, base, s[1], True, None)
                    pk[s][0] += t
                    pk[s][1] += l
        if nrecv["serial"] + nrecv["pairs"] == 0:
            continue                           # (every sampled receiver done, or under a done in-neighbour)
        tn, ln = now["serial"][0] + now["pairs"][0], now["serial"][1] + now["pairs"][1]
        cells = " | ".join(f"{pk[s][0]} ({100.0 * (pk[s][0] - now[s[0]][0]) / max(now[s[0]][0], 1):+.0f} %), "
                           f"{pk[s][1]} ({100.0 * (pk[s][1] - now[s[0]][1]) / max(now[s[0]][1], 1):+.1f} %)" for s in sweep)
        print(f"| {r} | {nrecv['serial']} / {nrecv['pairs']} | {tn} (serial {now['serial'][0]}, pairs {now['pairs'][0]}) | "
              f"{ln} (serial {now['serial'][1]}, pairs {now['pairs'][1]}) | {cells} | "
              f"{' / '.join(map(str, hist))} | {' / '.join(map(str, h1))} | {' / '.join(map(str, h2))} |", flush=True)


if __name__ == "__main__":
    main()
