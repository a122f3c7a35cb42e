"""The expected per-peer traffic totals of tests/load_ref.py against a
per-delivery replay, and load.py's helpers on hand-computed arrays (CPU).

load_ref reconstructs sent[] / recv[] from the C oracle's
first-receipt matrix, stats and reports.  The replay below shares nothing with
it but the crash draw: it runs the protocol peer by peer -- liveness with its
own miss counters and removals, injection, then a loop over senders, their
frontier and their out-links that appends every delivered line to the
receiver's inbox, as Peer.py:402-404 sends and Peer.py:206 / Peer.py:286 log.
sent[u] is the lines u wrote to links the seed had not dropped, recv[v] the
length of v's inbox log.
"""
import numpy as np
import pytest

import directed_shapes as ds
import load_ref


def replay(g, origin, inject, crashed_at, miss_threshold=3, max_rounds=254):
    n, m = int(g.n), len(origin)
    ins = [list(map(int, g.col[g.row_ptr[v]:g.row_ptr[v + 1]])) for v in range(n)]
    outs = [[] for _ in range(n)]
    for v in range(n):
        for u in ins[v]:
            outs[u].append(v)
    links = [ins[v] + (outs[v] if g.directed else []) for v in range(n)]
    up, removed, miss = [True] * n, [False] * n, [0] * n
    held = [set() for _ in range(n)]
    outbox = [[] for _ in range(n)]
    log = [[] for _ in range(n)]        # (round, sender, message) of every arrival
    sent = [0] * n
    per_round = []
    last = max(inject) if m else -1
    for r in range(max_rounds):
        for v in range(n):
            if up[v] and crashed_at[v] == r:
                up[v] = False
                outbox[v] = []
            if not up[v]:
                miss[v] += 1
        for v in range(n):
            if not up[v] and miss[v] == miss_threshold and not removed[v]:
                if any(up[u] and not removed[u] for u in links[v]):
                    removed[v] = True
        for k in range(m):
            if inject[k] == r and up[origin[k]]:
                held[origin[k]].add(k)
                outbox[origin[k]].append(k)
        inbox = [[] for _ in range(n)]
        for u in range(n):
            for k in outbox[u]:
                for w in outs[u]:
                    if removed[w]:
                        continue            # the seed dropped the link
                    sent[u] += 1
                    if up[w]:
                        inbox[w].append((r, u, k))
            outbox[u] = []
        new = 0
        for w in range(n):
            log[w].extend(inbox[w])
            for _, _, k in inbox[w]:
                if k not in held[w]:
                    held[w].add(k)
                    outbox[w].append(k)
                    new += 1
        per_round.append((np.array(sent, np.int64), np.array([len(x) for x in log], np.int64)))
        if new == 0 and r >= last:
            break
    return per_round, [len(h) for h in held]


def check(oracle, g, origin, inject, crashes=(), **churn):
    ref = oracle.run(g, origin, inject, crashes=crashes, want_first=True, **churn)
    exp = load_ref.totals(g, ref, crashes=crashes, **churn)
    got, held = replay(g, origin.tolist(), inject.tolist(), exp["crashed_at"].tolist())
    assert len(got) == ref["rounds"] == len(exp["per_round"])
    for r, ((s0, r0), (s1, r1)) in enumerate(zip(got, exp["per_round"])):
        assert np.array_equal(s0, s1), (r, np.nonzero(s0 != s1)[0][:8])
        assert np.array_equal(r0, r1), (r, np.nonzero(r0 != r1)[0][:8])
    assert np.array_equal(held, (ref["first"] != 255).sum(axis=1))
    assert int(exp["sent"].sum()) == sum(s["sends"] for s in ref["stats"])
    assert int(exp["recv"].sum()) <= int(exp["sent"].sum())
    cut = load_ref.totals(g, ref, crashes=crashes, rounds=2, **churn)
    assert np.array_equal(cut["sent"], got[1][0]) and np.array_equal(cut["recv"], got[1][1])
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
    assert int(exp["recv"].sum()) == int(exp["sent"].sum()) > 0
    # without liveness the totals are a function of the final Message-Lists
    held = (ref["first"] != 255).sum(axis=1)
    assert np.array_equal(exp["sent"], held * np.diff(g.row_ptr))
    assert np.array_equal(exp["recv"], load_ref.row_sums(g.row_ptr, g.col.astype(np.int64), held))


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
    assert int(exp["recv"].sum()) < int(exp["sent"].sum())


@pytest.mark.parametrize("directed", [False, True])
def test_churn(pkg, oracle, directed):
    g = ds.oriented_chung_lu(pkg, oracle, 200, 8, 2.2, 5, "coin") if directed else undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 4)
    ref, exp = check(oracle, g, origin, inject, churn=True, p_fail=0.05, churn_seed=11)
    assert sum(s["crashed"] for s in ref["stats"]) > 0 and sum(s["removals"] for s in ref["stats"]) > 0
    assert int(exp["recv"].sum()) < int(exp["sent"].sum())


def test_reconstruction_refuses_another_run(pkg, oracle):
    g = undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 20, 5)
    ref = oracle.run(g, origin, inject, crashes=[(int(origin[0]), 1)], want_first=True)
    with pytest.raises(AssertionError):
        load_ref.totals(g, ref)   # the crash left out: the oracle's sends do not match


# -- load.py ------------------------------------------------------------------

def test_duplicates(pkg):
    recv = np.array([10, 0, 7, 3], np.uint64)
    seenpop = np.array([4, 2, 3, 0], np.uint32)
    own = np.array([1, 2, 0, 0])
    dup = pkg.load.duplicates(recv, seenpop, own)
    assert dup.dtype == np.int64 and dup.tolist() == [7, 0, 4, 3]
    assert pkg.load.duplicates(np.zeros(3, np.uint64), np.zeros(3, np.uint32), np.zeros(3, np.int64)).tolist() == [0] * 3
    with pytest.raises(ValueError):
        pkg.load.duplicates(recv, seenpop, np.array([5, 0, 0, 0]))   # own > seenpop
    with pytest.raises(ValueError):
        pkg.load.duplicates(np.array([1, 0, 0, 0]), seenpop, own)    # fewer arrivals than first receipts
    with pytest.raises(ValueError):
        pkg.load.duplicates(recv[:3], seenpop, own)


def test_by_degree(pkg):
    # bins=4 over degrees up to 64: lower bounds 1, 4, 16, 64
    deg = np.array([1, 2, 3, 0, 64, 70 - 6, 1, 5])
    val = np.array([10, 20, 60, 999, 1000, 3000, 30, 7], np.uint64)
    lo, count, mean, vmax = pkg.load.by_degree(val, deg, bins=4)
    assert lo.tolist() == [1, 4, 16, 64]
    assert count.tolist() == [4, 1, 0, 2]          # class [16, 64) holds no vertex; degree 0 is in none
    assert mean.tolist() == [30.0, 7.0, 0.0, 2000.0]
    assert vmax.tolist() == [60, 7, 0, 3000]
    # the classes are those of degree.ccdf
    big = np.arange(1, 500)
    assert np.array_equal(pkg.load.by_degree(big, big)[0], pkg.degree.ccdf(big)[0])
    lo, count, mean, vmax = pkg.load.by_degree(np.zeros(8, np.uint64), deg, bins=4)
    assert count.tolist() == [4, 1, 0, 2] and not mean.any() and not vmax.any()
    lo, count, mean, vmax = pkg.load.by_degree(np.zeros(3), np.zeros(3, np.int64))
    assert lo.size == count.size == mean.size == vmax.size == 0
    with pytest.raises(ValueError):
        pkg.load.by_degree(val, deg[:4])


def test_concentration(pkg):
    v = np.array([1] * 99 + [101], np.uint64)         # total 200, mean 2
    c = pkg.load.concentration(v, top=0.01)
    assert c == {"top_share": 101 / 200, "max_over_mean": 101 / 2}
    c = pkg.load.concentration(v, top=0.02)
    assert c["top_share"] == 102 / 200
    assert pkg.load.concentration(v, top=1.0)["top_share"] == 1.0
    assert pkg.load.concentration(np.array([5, 1]), top=0.01)["top_share"] == 5 / 6   # at least one peer
    assert pkg.load.concentration(np.zeros(10, np.uint64)) == {"top_share": 0.0, "max_over_mean": 0.0}
    assert pkg.load.concentration(np.zeros(0)) == {"top_share": 0.0, "max_over_mean": 0.0}
    with pytest.raises(ValueError):
        pkg.load.concentration(v, top=0.0)
