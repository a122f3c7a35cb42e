"""The expected per-peer delay distributions of tests/delay_dist_ref.py against
a per-receipt replay (CPU), and the identities DESIGN.md §2.4 states for them.

delay_dist_ref evaluates the first-receipt formula on the C oracle's matrix.
The replay below shares nothing with it but the crash draw: it walks the rounds
with frontiers as sets and books every receipt at its receiver when it happens,
in the column of the delay read off the round counter -- the time column of the
reference's arrival log (Peer.py:206, Peer.py:286), kept per value.
"""
import numpy as np
import pytest

import delay_dist_ref
import delay_ref
import link_ref
import load_ref
from test_gpu_curve import _width_ref, histogram


def replay(g, origin, inject, crashed_at, max_rounds=254):
    n, m = int(g.n), len(origin)
    outs = [[] for _ in range(n)]
    for v in range(n):
        for j in range(int(g.row_ptr[v]), int(g.row_ptr[v + 1])):
            outs[int(g.col[j])].append(v)
    held = [set() for _ in range(n)]
    frontier = [set() for _ in range(n)]
    dist = [[0] * 16 for _ in range(n)]
    per_round = []
    last = max(inject) if m else -1
    for r in range(max_rounds):
        up = [crashed_at[v] > r for v in range(n)]
        for v in range(n):
            if not up[v]:
                frontier[v] = set()
        for k in range(m):
            if inject[k] == r and up[origin[k]] and k not in held[origin[k]]:   # a receipt with delay 0
                held[origin[k]].add(k)
                frontier[origin[k]].add(k)
                dist[origin[k]][0] += 1
        before = [set(h) for h in held]
        nxt = [set() for _ in range(n)]
        for u in range(n):
            for k in frontier[u]:
                for w in outs[u]:
                    if up[w] and k not in before[w] and k not in nxt[w]:
                        nxt[w].add(k)
                        d = r + 1 - inject[k]      # received in round r: receipt round r + 1
                        assert d >= 1
                        dist[w][min(d, 15)] += 1
        new = 0
        for w in range(n):
            held[w] |= nxt[w]
            new += len(nxt[w])
        frontier = nxt
        per_round.append(np.array(dist, np.int64))
        if new == 0 and r >= last:
            break
    return per_round


def check(oracle, g, origin, inject, crashes=()):
    ref = oracle.run(g, origin, inject, crashes=crashes, want_first=True)
    exp = delay_dist_ref.totals(ref, inject)
    crashed_at = load_ref.crash_rounds(int(g.n), ref["rounds"], crashes, False, 0.0, 0)
    got = replay(g, origin.tolist(), inject.tolist(), crashed_at.tolist())
    assert len(got) == ref["rounds"] == len(exp["per_round"])
    for r in range(ref["rounds"]):
        dist, sp = exp["per_round"][r]
        assert np.array_equal(got[r], dist), r
        assert np.array_equal(dist.sum(axis=1), sp)
    assert np.array_equal(got[-1], exp["dist"])
    assert np.array_equal(delay_dist_ref.totals(ref, inject, rounds=2)["dist"], got[1])
    return ref, exp


def identities(pkg, ref, inject, exp):
    """the "Consequences" of DESIGN.md §2.4, against delay_ref.totals"""
    old = delay_ref.totals(ref, inject)
    dist = exp["dist"]
    assert np.array_equal(dist.sum(axis=1), old["seenpop"]) and np.array_equal(exp["seenpop"], old["seenpop"])
    weighted = (dist * np.arange(16)).sum(axis=1)
    top = np.where(dist > 0, np.arange(16)[None, :], 0).max(axis=1)
    open_ = dist[:, 15] == 0
    assert np.array_equal(weighted[open_], old["sum"][open_]) and np.array_equal(top[open_], old["max"][open_])
    assert (weighted[~open_] <= old["sum"][~open_]).all() and (old["max"][~open_] >= 15).all()
    pkg.latency.dist_check(dist, old["seenpop"], old["sum"], old["max"])
    for r in range(len(exp["per_round"])):
        d, sp = exp["per_round"][r]
        s, mx, sp2 = old["per_round"][r]
        pkg.latency.dist_check(d, sp2, s, mx)
        assert np.array_equal(sp, sp2)
    return open_


def small(pkg, oracle):
    rp, col = oracle.chung_lu(30, 3, 2.2, 3)
    return pkg.CSR(30, rp, col, False)


def test_replay_staggered_injects(pkg, oracle):
    g = small(pkg, oracle)
    origin = pkg.overlay.random_origins(g.n, 40, seed=1)
    inject = (np.arange(40) * 3 % 7).astype(np.int32)
    ref, exp = check(oracle, g, origin, inject)
    assert int(exp["dist"][:, 0].sum()) == 40 and (exp["dist"][:, 1:].sum(axis=0) > 0).sum() >= 3
    assert identities(pkg, ref, inject, exp).all()


def test_replay_with_crashes(pkg, oracle):
    g = small(pkg, oracle)
    origin = pkg.overlay.random_origins(g.n, 40, seed=2)
    inject = (np.arange(40) % 4).astype(np.int32)
    plain = oracle.run(g, origin, inject, want_first=True)
    # crash right after a receipt from a neighbour (no injection): it still received
    got2 = np.nonzero(((plain["first"] == 2) & (inject != 2)[None, :]).any(axis=1))[0][:3]
    hub = int(np.argmax(np.diff(g.row_ptr)))
    crashes = [(int(v), 2) for v in got2] + [(hub, 1), (int(origin[5]), 0)]
    ref, exp = check(oracle, g, origin, inject, crashes=crashes)
    assert (exp["dist"][got2, 1:].sum(axis=1) > 0).any()
    assert int(exp["dist"][:, 0].sum()) < 40   # the down origin's injections were lost
    assert not np.array_equal(exp["dist"], delay_dist_ref.totals(plain, inject)["dist"])
    identities(pkg, ref, inject, exp)


@pytest.mark.parametrize("m", [1, 7, 4096])
def test_path_saturates(pkg, oracle, m):
    """a path of 24 peers with every message injected at vertex 0 in round 0:
    vertex v hears each of them v rounds later -- columns 1 .. 14 hold one peer
    each, column 15 the last 9 hops"""
    g = link_ref.path(pkg, 24)
    origin, inject = np.zeros(m, np.int32), np.zeros(m, np.int32)
    ref = oracle.run(g, origin, inject, want_first=True)
    exp = delay_dist_ref.totals(ref, inject)
    want = np.zeros((24, 16), np.int64)
    for v in range(24):
        want[v, min(v, 15)] = m
    assert np.array_equal(exp["dist"], want)
    assert exp["dist"].sum(axis=0).tolist() == [m] * 15 + [9 * m]
    open_ = identities(pkg, ref, inject, exp)
    assert open_.tolist() == [True] * 15 + [False] * 9
    t = delay_dist_ref.bins(g, exp["dist"])
    assert t[0].tolist() == [m] + [0] * 14 + [m] and int(t[1].sum()) == 22 * m and not t[2:].any()
    assert np.array_equal(t, pkg.latency.dist_bins(np.diff(g.row_ptr), exp["dist"]))


def test_curve_and_bins_identities(pkg, oracle):
    """sum_v delay_dist[v][d] = delay_hist[d] (d <= 14), column 15 its tail;
    the table's row sums are delay_bins' receipts"""
    g, origin, inject, ref = _width_ref(4099, 100)
    exp = delay_dist_ref.totals(ref, inject)
    identities(pkg, ref, inject, exp)
    curve = histogram(ref["first"], ref["rounds"] + 1)
    hist = pkg.latency.delay_hist(curve, inject).astype(np.int64)
    hist = np.concatenate([hist, np.zeros(max(0, 16 - hist.size), np.int64)])
    cols = exp["dist"].sum(axis=0)
    assert np.array_equal(cols[:15], hist[:15]) and int(cols[15]) == int(hist[15:].sum())
    assert int(cols[0]) == 100
    t = delay_dist_ref.bins(g, exp["dist"])
    assert np.array_equal(t, pkg.latency.dist_bins(np.diff(g.row_ptr), exp["dist"]))
    assert np.array_equal(t.sum(axis=1), delay_ref.bins(g, ref, inject)[:, 2])
    half = delay_dist_ref.bins(g, exp["dist"], lo=1000, hi=3000) + delay_dist_ref.bins(g, exp["dist"], hi=1000) + \
        delay_dist_ref.bins(g, exp["dist"], lo=3000)
    assert np.array_equal(half, t)
    # hubs hear early: the top bin's median is no later than the leaves', its tail earlier
    rows = pkg.latency.dist_by_degree(t)
    assert rows[-1]["p50"] <= rows[1]["p50"] and rows[-1]["p99"] < rows[1]["p99"]


def test_shards_add_up(pkg, oracle):
    g = small(pkg, oracle)
    origin = pkg.overlay.random_origins(g.n, 128, seed=4)
    inject = (np.arange(128) % 5).astype(np.int32)
    whole = delay_dist_ref.totals(oracle.run(g, origin, inject, want_first=True), inject)
    parts = [delay_dist_ref.totals(oracle.run(g, origin[a:b], inject[a:b], want_first=True), inject[a:b])
             for a, b in [(0, 64), (64, 128)]]
    both = pkg.latency.dist_combine([p["dist"].astype(np.uint16) for p in parts])
    assert both.dtype == np.int64 and np.array_equal(both, whole["dist"])
