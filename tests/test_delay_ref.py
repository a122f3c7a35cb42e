"""The expected per-peer receipt delays of tests/delay_ref.py against a
per-receipt replay (CPU), and the identities DESIGN.md §2.4 states for them.

delay_ref evaluates the first-receipt formula on the C oracle's matrix.  The
replay below shares nothing with it but the crash draw: it walks the rounds
with frontiers as sets and books every first receipt at its receiver when it
happens, with the delay read off the round counter -- the time column of the
reference's arrival log (Peer.py:206, Peer.py:286).
"""
import numpy as np
import pytest

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
    dsum, dmax = [0] * n, [0] * n
    per_round = []
    last = max(inject) if m else -1
    for r in range(max_rounds):
        up = [crashed_at[v] > r for v in range(n)]
        for v in range(n):
            if not up[v]:
                frontier[v] = set()
        for k in range(m):
            if inject[k] == r and up[origin[k]]:   # a receipt with delay 0
                held[origin[k]].add(k)
                frontier[origin[k]].add(k)
        before = [set(h) for h in held]
        nxt = [set() for _ in range(n)]
        for u in range(n):
            for k in frontier[u]:
                for w in outs[u]:
                    if up[w] and k not in before[w] and k not in nxt[w]:
                        nxt[w].add(k)
                        d = r + 1 - inject[k]      # received in round r: receipt round r + 1
                        assert d >= 1
                        dsum[w] += d
                        dmax[w] = max(dmax[w], d)
        new = 0
        for w in range(n):
            held[w] |= nxt[w]
            new += len(nxt[w])
        frontier = nxt
        per_round.append((np.array(dsum, np.int64), np.array(dmax, np.int64),
                          np.array([len(h) for h in held], np.int64)))
        if new == 0 and r >= last:
            break
    return per_round


def check(oracle, g, origin, inject, crashes=()):
    ref = oracle.run(g, origin, inject, crashes=crashes, want_first=True)
    exp = delay_ref.totals(ref, inject)
    crashed_at = load_ref.crash_rounds(int(g.n), ref["rounds"], crashes, False, 0.0, 0)
    got = replay(g, origin.tolist(), inject.tolist(), crashed_at.tolist())
    assert len(got) == ref["rounds"] == len(exp["per_round"])
    for r in range(ref["rounds"]):
        for a, b in zip(got[r], exp["per_round"][r]):
            assert np.array_equal(a, b), r
    for a, b in zip(got[-1], (exp["sum"], exp["max"], exp["seenpop"])):
        assert np.array_equal(a, b)
    cut = delay_ref.totals(ref, inject, rounds=2)
    assert np.array_equal(cut["sum"], got[1][0]) and np.array_equal(cut["max"], got[1][1])
    return ref, exp


def small(pkg, oracle):
    rp, col = oracle.chung_lu(30, 3, 2.2, 3)
    return pkg.CSR(30, rp, col, False)


def test_replay_staggered_injects(pkg, oracle):
    g = small(pkg, oracle)
    origin = pkg.overlay.random_origins(g.n, 40, seed=1)
    inject = (np.arange(40) * 3 % 7).astype(np.int32)
    ref, exp = check(oracle, g, origin, inject)
    assert exp["max"].max() >= 3 and len(set(exp["max"].tolist())) >= 3
    assert (exp["seenpop"] == 0).any() or (np.diff(g.row_ptr) > 0).all()
    # an origin holds its own message with delay 0: seenpop counts it, the sum does not
    assert np.array_equal(exp["seenpop"], (ref["first"] != 255).sum(axis=1))


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
    assert (exp["sum"][got2] > 0).any()   # (the other crashes may have cut one of them off)
    assert not np.array_equal(exp["sum"], delay_ref.totals(plain, inject)["sum"])


@pytest.mark.parametrize("m", [1, 7, 4096])
def test_path_closed_form(pkg, oracle, m):
    """the path 0-1-2-3-4 with every message injected at vertex 0 in round 0:
    vertex v hears each of them v rounds later"""
    g = link_ref.path(pkg, 5)
    origin, inject = np.zeros(m, np.int32), np.zeros(m, np.int32)
    ref = oracle.run(g, origin, inject, want_first=True)
    exp = delay_ref.totals(ref, inject)
    assert exp["sum"].tolist() == [m * v for v in range(5)]
    assert exp["max"].tolist() == list(range(5))
    assert exp["seenpop"].tolist() == [m] * 5
    assert np.array_equal(delay_ref.totals(ref, None)["sum"], exp["sum"])
    t = delay_ref.bins(g, ref, inject)
    assert t[0].tolist() == [2, 2, 2 * m, 4 * m, 4] and t[1].tolist() == [3, 3, 3 * m, 6 * m, 3] and not t[2:].any()
    assert np.array_equal(t, pkg.latency.bins(np.diff(g.row_ptr), exp["seenpop"], exp["sum"], exp["max"]))


def test_curve_identity(pkg, oracle):
    """sum_v delay_sum[v] = sum_R sum_k (R - inject[k]) * curve[R][k]"""
    g, origin, inject, ref = _width_ref(4099, 100)
    exp = delay_ref.totals(ref, inject)
    curve = histogram(ref["first"], ref["rounds"] + 1)
    assert int(exp["sum"].sum()) == pkg.latency.total_delay(curve, inject) > 0
    hist = pkg.latency.delay_hist(curve, inject)
    assert int(hist.sum()) == int(exp["seenpop"].sum()) and int(hist[0]) == 100
    assert int(np.nonzero(hist)[0].max()) == int(exp["max"].max())
    for r in (0, 1, ref["rounds"] - 1):   # ... and after every round
        s, mx, sp = exp["per_round"][r]
        assert int(s.sum()) == pkg.latency.total_delay(curve[:r + 2], inject)
    # what test_gpu_delay.py may assert of this shape
    deg = np.diff(g.row_ptr)
    assert (deg == 0).sum() > 100 and deg.max() > 512 and len(set(exp["max"].tolist())) >= 6
    t = delay_ref.bins(g, ref, inject)
    assert (t[:10, 0] > 0).all() and not t[10:].any()
    assert np.array_equal(t, pkg.latency.bins(deg, exp["seenpop"], exp["sum"], exp["max"]))
    # hubs hear early: the top bin's mean delay is below the leaves'
    rows = pkg.latency.by_degree(t)
    assert rows[-1]["mean_delay"] < rows[1]["mean_delay"]


def test_shards_add_up(pkg, oracle):
    g = small(pkg, oracle)
    origin = pkg.overlay.random_origins(g.n, 128, seed=4)
    inject = (np.arange(128) % 5).astype(np.int32)
    whole = delay_ref.totals(oracle.run(g, origin, inject, want_first=True), inject)
    parts = [delay_ref.totals(oracle.run(g, origin[a:b], inject[a:b], want_first=True), inject[a:b])
             for a, b in [(0, 64), (64, 128)]]
    assert np.array_equal(parts[0]["sum"] + parts[1]["sum"], whole["sum"])
    assert np.array_equal(np.maximum(parts[0]["max"], parts[1]["max"]), whole["max"])
    assert np.array_equal(parts[0]["seenpop"] + parts[1]["seenpop"], whole["seenpop"])
