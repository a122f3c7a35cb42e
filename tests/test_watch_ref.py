"""The expected watched-peers record of tests/watch_ref.py against a
per-delivery replay (CPU), and the identities DESIGN.md §2.4 states for it.

watch_ref evaluates the first-receipt formula on the C oracle's matrix.  The
replay below shares nothing with it but the crash draw: it walks the rounds with
frontiers as sets and every arc by its index in the in-CSR, and writes an
arrival into its (arc, message) cell when the receiver is up, duplicates
included -- the lines of the reference peer's log (Peer.py:206).  Every vertex
is watched, so the identities are checked on the oracle alone: the summaries of
the record are load_ref's recv, fresh_ref's recv, link_ref per arc, mult_ref's
sole_recv and delay_dist_ref's rows.
"""
import numpy as np
import pytest

import delay_dist_ref
import directed_shapes as ds
import fresh_ref
import link_ref
import load_ref
import mult_ref
import raw_csr
import watch_ref


def replay(g, origin, inject, crashed_at, max_rounds=254):
    n, m = int(g.n), len(origin)
    outs = [[] for _ in range(n)]           # u -> [(v, arc index)]
    for v in range(n):
        for j in range(int(g.row_ptr[v]), int(g.row_ptr[v + 1])):
            outs[int(g.col[j])].append((v, j))
    first = np.full((n, m), 255, np.uint8)
    arrival = np.full((int(g.row_ptr[n]), m), 255, np.uint8)
    frontier = [set() for _ in range(n)]
    per_round = []
    last = max(inject) if m else -1
    for r in range(max_rounds):
        up = [crashed_at[v] > r for v in range(n)]
        for v in range(n):
            if not up[v]:
                frontier[v] = set()          # crash-stop: the frontier is dropped
        for k in range(m):
            if inject[k] == r and up[origin[k]]:
                first[origin[k], k] = r
                frontier[origin[k]].add(k)
        held = first != 255                  # what every peer holds at the start of E_r
        nxt = [set() for _ in range(n)]
        for u in range(n):
            for k in frontier[u]:
                for w, j in outs[u]:
                    if up[w]:                # the line arrives, news or not
                        assert arrival[j, k] == 255
                        arrival[j, k] = r + 1
                        if not held[w, k]:
                            nxt[w].add(k)
        new = 0
        for w in range(n):
            for k in nxt[w]:
                first[w, k] = r + 1
            new += len(nxt[w])
        frontier = nxt
        per_round.append((first.copy(), arrival.copy()))
        if new == 0 and r >= last:
            break
    return per_round


def check(oracle, g, origin, inject, crashes=(), **churn):
    ref = oracle.run(g, origin, inject, crashes=crashes, want_first=True, **churn)
    everyone = list(range(int(g.n)))
    rec = watch_ref.record(g, ref, everyone, crashes=crashes, **churn)
    got = replay(g, origin.tolist(), inject.tolist(), rec["crashed_at"].tolist())
    assert len(got) == ref["rounds"]
    assert np.array_equal(got[-1][0], ref["first"])
    assert np.array_equal(rec["ptr"], np.asarray(g.row_ptr, np.int64))           # every vertex watched: the in-CSR itself
    assert np.array_equal(got[-1][1], rec["arrival"]), np.argwhere(got[-1][1] != rec["arrival"])[:8]
    for r, (f, a) in enumerate(got):                                              # and between rounds
        cf, ca = watch_ref.after(rec, r + 1, origin, inject)
        assert np.array_equal(f, cf) and np.array_equal(a, ca), r
    # the identities, on the oracle alone
    kw = dict(crashes=crashes, **churn)
    sm = watch_ref.summaries(rec)
    assert np.array_equal([s["lines"] for s in sm], load_ref.totals(g, ref, **kw)["recv"])
    assert np.array_equal([s["fresh"] for s in sm], fresh_ref.totals(g, ref, **kw)["recv"])
    assert np.array_equal(np.concatenate([s["arc_fresh"] for s in sm]), link_ref.record(g, ref, **kw)["link"])
    assert np.array_equal([s["sole"] for s in sm], mult_ref.totals(g, ref, **kw)["sole_recv"])
    dd = delay_dist_ref.totals(ref, inject)
    assert np.array_equal([s["held"] for s in sm], dd["seenpop"])
    for v in range(int(g.n)):
        held = rec["first"][v] != 255
        d = np.minimum(rec["first"][v][held].astype(np.int64) - np.asarray(inject, np.int64)[held], 15)
        assert np.array_equal(np.bincount(d, minlength=16), np.asarray(dd["dist"][v], np.int64)), v
    got_a = rec["arrival"] != 255
    assert (rec["first"][rec["slot"]][got_a] <= rec["arrival"][got_a]).all()
    return ref, rec


def messages(pkg, g, m, seed):
    return pkg.overlay.random_origins(g.n, m, seed=seed), (np.arange(m) % 3).astype(np.int32)


def undirected(pkg, oracle, n=200):
    rp, col = oracle.chung_lu(n, 4, 2.2, 3)
    return pkg.CSR(n, rp, col, False)


def test_undirected_nobody_down(pkg, oracle):
    g = undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 1)
    ref, rec = check(oracle, g, origin, inject)
    fresh = (rec["arrival"] == rec["first"][rec["slot"]]) & (rec["arrival"] != 255)
    assert fresh.sum() > sum(s["new_bits"] for s in ref["stats"]) > 0           # some message came twice at once
    assert ((rec["arrival"] != 255) & ~fresh).any()                             # and duplicates came later


def test_raw_csr(pkg, oracle):
    g = raw_csr.loops_and_repeats(pkg)
    origin, inject = messages(pkg, g, 6, 41)
    ref, rec = check(oracle, g, origin, inject)
    loop = np.nonzero(rec["sender"] == rec["slot"])[0]
    assert loop.size == 300
    f = rec["first"][rec["slot"][loop]]
    assert np.array_equal(rec["arrival"][loop], np.where(f != 255, f + 1, 255))   # a self-loop: a row of duplicates


def test_directed(pkg, oracle):
    g = ds.oriented_chung_lu(pkg, oracle, 200, 6, 2.2, 5, "coin")
    assert g.directed
    origin, inject = messages(pkg, g, 64, 2)
    check(oracle, g, origin, inject)


def test_explicit_crashes(pkg, oracle):
    g = undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 3)
    plain = oracle.run(g, origin, inject, want_first=True)
    hub = int(np.argmax(np.diff(g.row_ptr)))
    got2 = np.nonzero((plain["first"] == 2).any(axis=1))[0][:5]   # crash right after a receipt
    crashes = [(hub, 1)] + [(int(v), 2) for v in got2] + [(int(origin[3]), 0), (hub, 4)]
    ref, rec = check(oracle, g, origin, inject, crashes=crashes)
    assert sum(s["removals"] for s in ref["stats"]) > 0 and sum(s["lost"] for s in ref["stats"]) > 0
    a = rec["arrival"][rec["slot"] == hub]
    assert (a[a != 255] <= 1).all()                                # nothing arrives at a crashed peer


def test_churn_with_removals(pkg, oracle):
    g = undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 4)
    ref, _ = check(oracle, g, origin, inject, churn=True, p_fail=0.02, churn_seed=11)
    assert sum(s["crashed"] for s in ref["stats"]) > 0 and sum(s["removals"] for s in ref["stats"]) > 0
