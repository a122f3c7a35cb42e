"""The expected fresh deliveries of tests/fresh_ref.py against a per-delivery
replay (CPU), and the identities DESIGN.md §2.4 states for them.

fresh_ref evaluates the first-receipt formula on the C oracle's matrix.  The
replay below shares nothing with it but the crash draw: it walks the rounds
with frontiers as sets and every arc, and counts an arrival as fresh when the
receiver is up and does not hold the message at the start of the round --
several neighbours delivering one message in one round all count.
"""
import numpy as np
import pytest

import directed_shapes as ds
import fresh_ref
import load_ref


def replay(g, origin, inject, crashed_at, max_rounds=254):
    n, m = int(g.n), len(origin)
    outs = [[] for _ in range(n)]
    for v in range(n):
        for u in g.col[g.row_ptr[v]:g.row_ptr[v + 1]].tolist():
            outs[u].append(v)
    held = [set() for _ in range(n)]
    frontier = [set() for _ in range(n)]
    fresh_sent, fresh_recv = [0] * n, [0] * n
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
                for w in outs[u]:
                    if up[w] and k not in before[w]:
                        fresh_sent[u] += 1
                        fresh_recv[w] += 1
                        nxt[w].add(k)
        new = 0
        for w in range(n):
            held[w] |= nxt[w]
            new += len(nxt[w])
        frontier = nxt
        news.append(new)
        per_round.append((np.array(fresh_sent, np.int64), np.array(fresh_recv, np.int64)))
        if new == 0 and r >= last:
            break
    return per_round, news


def check(oracle, g, origin, inject, crashes=(), **churn):
    ref = oracle.run(g, origin, inject, crashes=crashes, want_first=True, **churn)
    exp = fresh_ref.totals(g, ref, crashes=crashes, **churn)
    got, news = replay(g, origin.tolist(), inject.tolist(), exp["crashed_at"].tolist())
    assert len(got) == ref["rounds"] == len(exp["per_round"])
    assert news == [s["new_bits"] for s in ref["stats"]]
    for r, ((s0, r0), (s1, r1)) in enumerate(zip(got, exp["per_round"])):
        assert np.array_equal(s0, s1), (r, np.nonzero(s0 != s1)[0][:8])
        assert np.array_equal(r0, r1), (r, np.nonzero(r0 != r1)[0][:8])
    cut = fresh_ref.totals(g, ref, crashes=crashes, rounds=2, **churn)
    assert np.array_equal(cut["sent"], got[1][0]) and np.array_equal(cut["recv"], got[1][1])
    identities(g, origin, ref, exp, load_ref.totals(g, ref, crashes=crashes, **churn))
    return ref, exp


def identities(g, origin, ref, exp, load):
    """the consequences DESIGN.md §2.4 lists"""
    assert int(exp["sent"].sum()) == int(exp["recv"].sum())
    assert (exp["sent"] <= load["sent"]).all() and (exp["recv"] <= load["recv"]).all()
    first = ref["first"]
    m = first.shape[1]
    injected = first[origin, np.arange(m)] != 255          # (a message lost at a down origin never existed)
    own = np.bincount(origin[injected], minlength=g.n)
    arrived = (first != 255).sum(axis=1) - own
    assert (exp["recv"] >= arrived).all()
    prev = 0
    for r, (_, rv) in enumerate(exp["per_round"]):
        assert int(rv.sum()) - prev >= ref["stats"][r]["new_bits"], r
        prev = int(rv.sum())
    return arrived


def messages(pkg, g, m, seed):
    return pkg.overlay.random_origins(g.n, m, seed=seed), (np.arange(m) % 4).astype(np.int32)


def undirected(pkg, oracle, n=200):
    rp, col = oracle.chung_lu(n, 4, 2.2, 3)
    return pkg.CSR(n, rp, col, False)


def test_undirected_nobody_down(pkg, oracle):
    g = undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 1)
    ref, exp = check(oracle, g, origin, inject)
    assert int(exp["recv"].sum()) > sum(s["new_bits"] for s in ref["stats"]) > 0   # some message came twice at once


def test_one_deliverer_each_is_equality(pkg, oracle):
    """a path: every message reaches every peer from one neighbour only, so
    fresh_recv is exactly the first receipts and nothing else is fresh"""
    n = 9
    rp = np.array([0] + [1 if v in (0, n - 1) else 2 for v in range(n)], np.int64).cumsum()
    col = np.array([u for v in range(n) for u in (v - 1, v + 1) if 0 <= u < n], np.int32)
    g = pkg.CSR(n, rp, col, False)
    origin, inject = np.array([0, 4, 8], np.int32), np.array([0, 1, 0], np.int32)
    ref, exp = check(oracle, g, origin, inject)
    own = np.bincount(origin, minlength=n)
    assert np.array_equal(exp["recv"], (ref["first"] != 255).sum(axis=1) - own)
    assert int(exp["recv"].sum()) == sum(s["new_bits"] for s in ref["stats"])


def test_two_deliverers_in_one_round_both_count(pkg, oracle):
    """a 4-cycle: the vertex opposite the origin gets the message from both of
    its neighbours in the same round"""
    rp = np.array([0, 2, 4, 6, 8], np.int64)
    col = np.array([1, 3, 0, 2, 1, 3, 0, 2], np.int32)
    g = pkg.CSR(4, rp, col, False)
    ref, exp = check(oracle, g, np.array([0], np.int32), np.array([0], np.int32))
    assert exp["recv"].tolist() == [0, 1, 2, 1] and exp["sent"].tolist() == [2, 1, 0, 1]


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
    # a vertex that crashed in the round it would have sent delivered nothing of that receipt
    plain_exp = fresh_ref.totals(g, plain)
    assert int(exp["sent"][got2].sum()) < int(plain_exp["sent"][got2].sum())


@pytest.mark.parametrize("directed", [False, True])
def test_churn(pkg, oracle, directed):
    g = ds.oriented_chung_lu(pkg, oracle, 200, 8, 2.2, 5, "coin") if directed else undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 4)
    ref, exp = check(oracle, g, origin, inject, churn=True, p_fail=0.05, churn_seed=11)
    assert sum(s["crashed"] for s in ref["stats"]) > 0 and sum(s["removals"] for s in ref["stats"]) > 0
