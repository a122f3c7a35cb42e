"""The expected per-link fresh deliveries of tests/link_ref.py against a
per-delivery replay (CPU), and the identities DESIGN.md §2.4 states for them.

link_ref evaluates the first-receipt formula on the C oracle's matrix.  The
replay below shares nothing with it but the crash draw: it walks the rounds
with frontiers as sets and every arc by its index in the in-CSR, and books an
arrival on its arc when the receiver is up and does not hold the message at the
start of the round -- several neighbours delivering one message in one round
all count, each on its own arc.
"""
import numpy as np
import pytest

import directed_shapes as ds
import fresh_curve_ref
import fresh_ref
import link_ref
from test_gpu_curve import _width_ref


def replay(g, origin, inject, crashed_at, max_rounds=254):
    n, m = int(g.n), len(origin)
    outs = [[] for _ in range(n)]           # u -> [(v, arc index)]
    for v in range(n):
        for j in range(int(g.row_ptr[v]), int(g.row_ptr[v + 1])):
            outs[int(g.col[j])].append((v, j))
    held = [set() for _ in range(n)]
    frontier = [set() for _ in range(n)]
    link = [0] * int(g.row_ptr[n])
    per_round, news = [], []
    last = max(inject) if m else -1
    for r in range(max_rounds):
        up = [crashed_at[v] > r for v in range(n)]
        for v in range(n):
            if not up[v]:
                frontier[v] = set()          # crash-stop: the frontier is dropped
        for k in range(m):
            if inject[k] == r and up[origin[k]]:
                held[origin[k]].add(k)
                frontier[origin[k]].add(k)
        before = [set(h) for h in held]      # what every peer holds at the start of E_r
        nxt = [set() for _ in range(n)]
        for u in range(n):
            for k in frontier[u]:
                for w, j in outs[u]:
                    if up[w] and k not in before[w]:
                        link[j] += 1
                        nxt[w].add(k)
        new = 0
        for w in range(n):
            held[w] |= nxt[w]
            new += len(nxt[w])
        frontier = nxt
        news.append(new)
        per_round.append(np.array(link, np.int64))
        if new == 0 and r >= last:
            break
    return per_round, news


def identities(g, ref, exp, **kw):
    """the consequences DESIGN.md §2.4 lists, all exact"""
    tot = fresh_ref.totals(g, ref, **kw)
    n = int(g.n)
    for r, link in enumerate(exp["per_round"]):
        sent, recv = tot["per_round"][r]
        assert np.array_equal(np.bincount(exp["src"], weights=link, minlength=n).astype(np.int64), sent), r
        assert np.array_equal(np.bincount(exp["dst"], weights=link, minlength=n).astype(np.int64), recv), r
    fc = fresh_curve_ref.curve(g, ref, **kw)["curve"]
    assert int(exp["link"].sum()) == int(tot["recv"].sum()) == int(fc.sum())
    assert exp["link"].max(initial=0) <= ref["first"].shape[1]


def check(oracle, g, origin, inject, crashes=(), **churn):
    ref = oracle.run(g, origin, inject, crashes=crashes, want_first=True, **churn)
    exp = link_ref.record(g, ref, crashes=crashes, **churn)
    got, news = replay(g, origin.tolist(), inject.tolist(), exp["crashed_at"].tolist())
    assert len(got) == ref["rounds"] == len(exp["per_round"])
    assert news == [s["new_bits"] for s in ref["stats"]]
    for r, (a, b) in enumerate(zip(got, exp["per_round"])):
        assert np.array_equal(a, b), (r, np.nonzero(a != b)[0][:8])
    cut = link_ref.record(g, ref, crashes=crashes, rounds=2, **churn)
    assert np.array_equal(cut["link"], got[1])
    identities(g, ref, exp, crashes=crashes, **churn)
    return ref, exp


def messages(pkg, g, m, seed):
    return pkg.overlay.random_origins(g.n, m, seed=seed), (np.arange(m) % 4).astype(np.int32)


def undirected(pkg, oracle, n=200):
    rp, col = oracle.chung_lu(n, 4, 2.2, 3)
    return pkg.CSR(n, rp, col, False)


def test_undirected_nobody_down(pkg, oracle):
    g = undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 1)
    ref, exp = check(oracle, g, origin, inject)
    assert int(exp["link"].sum()) > sum(s["new_bits"] for s in ref["stats"]) > 0   # some message came twice at once
    assert (exp["link"] == 0).any() and (exp["link"] > 1).any()


def test_two_deliverers_in_one_round_both_count(pkg, oracle):
    """a 4-cycle: the vertex opposite the origin gets the message over both of
    its in-arcs in the same round, and nothing ever travels back"""
    rp = np.array([0, 2, 4, 6, 8], np.int64)
    col = np.array([1, 3, 0, 2, 1, 3, 0, 2], np.int32)
    g = pkg.CSR(4, rp, col, False)
    ref, exp = check(oracle, g, np.array([0], np.int32), np.array([0], np.int32))
    # arcs in CSR order: 1>0 3>0 | 0>1 2>1 | 1>2 3>2 | 0>3 2>3
    assert exp["link"].tolist() == [0, 0, 1, 0, 1, 1, 1, 0]


@pytest.mark.parametrize("m", [3, 4096])
def test_path_saturates(pkg, oracle, m):
    """the path 0-1-2-3-4 with every message injected at vertex 0: every arc
    pointing away from 0 carries all of them, every arc pointing back none --
    with 4,096 messages the u16 record's bound, attained"""
    g = link_ref.path(pkg, 5)
    origin, inject = np.zeros(m, np.int32), np.zeros(m, np.int32)
    ref = oracle.run(g, origin, inject, want_first=True)
    exp = link_ref.record(g, ref)
    away = exp["src"] < exp["dst"]
    assert away.sum() == 4 and (exp["link"][away] == m).all() and (exp["link"][~away] == 0).all()
    identities(g, ref, exp)
    if m == 3:
        got, _ = replay(g, origin.tolist(), inject.tolist(), exp["crashed_at"].tolist())
        assert np.array_equal(got[-1], exp["link"])


@pytest.mark.parametrize("kind", ["first3", "coin", "down"])
def test_directed(pkg, oracle, kind):
    g = ds.first3(pkg, 150) if kind == "first3" else ds.oriented_chung_lu(pkg, oracle, 200, 6, 2.2, 5, kind)
    assert g.directed and not np.array_equal(np.diff(g.row_ptr), np.bincount(g.col, minlength=g.n))
    origin, inject = messages(pkg, g, 64, 2)
    check(oracle, g, origin, inject)
    hub = int(np.argmax(np.bincount(g.col, minlength=g.n)))
    ref, exp = check(oracle, g, origin, inject, crashes=[(hub, 1), (int(origin[0]), 2)])
    assert sum(s["removals"] for s in ref["stats"]) > 0


def test_explicit_crashes(pkg, oracle):
    g = undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 3)
    plain = oracle.run(g, origin, inject, want_first=True)
    hub = int(np.argmax(np.diff(g.row_ptr)))
    got2 = np.nonzero((plain["first"] == 2).any(axis=1))[0][:5]   # crash right after a receipt
    crashes = [(hub, 1)] + [(int(v), 2) for v in got2] + [(int(origin[3]), 0), (hub, 4)]
    ref, exp = check(oracle, g, origin, inject, crashes=crashes)
    assert sum(s["removals"] for s in ref["stats"]) > 0 and sum(s["lost"] for s in ref["stats"]) > 0
    # a vertex that crashed in the round it would have sent delivered nothing of that receipt over its out-arcs,
    # and its in-arcs keep what they delivered
    plain_exp = link_ref.record(g, plain)
    out_arcs = np.isin(exp["src"], got2)
    assert int(exp["link"][out_arcs].sum()) < int(plain_exp["link"][out_arcs].sum())
    assert int(exp["link"][np.isin(exp["dst"], got2)].sum()) > 0


@pytest.mark.parametrize("directed", [False, True])
def test_churn(pkg, oracle, directed):
    g = ds.oriented_chung_lu(pkg, oracle, 200, 8, 2.2, 5, "coin") if directed else undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 4)
    ref, exp = check(oracle, g, origin, inject, churn=True, p_fail=0.05, churn_seed=11)
    assert sum(s["crashed"] for s in ref["stats"]) > 0 and sum(s["removals"] for s in ref["stats"]) > 0


@pytest.mark.parametrize("m", [100, 4096])
def test_width_shapes(pkg, oracle, m):
    """the shapes test_gpu_link_fresh.py runs: folds and totals against
    fresh_ref / fresh_curve_ref, and what its cases may assert of them"""
    g, origin, inject, ref = _width_ref(4099, m)
    exp = link_ref.record(g, ref)
    identities(g, ref, exp)
    link = exp["link"]
    assert (link == 0).any() and (link > 1).any() and link.max() <= m
    u, v, uv, vu = pkg.links.undirected(g, link)
    assert u.size * 2 == link.size and ((uv > 0) & (vu > 0)).any()   # some link has news in both directions
