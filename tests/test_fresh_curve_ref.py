"""The expected fresh-delivery curves of tests/fresh_curve_ref.py against a
per-delivery replay (CPU), the identities DESIGN.md §2.4 states for them, a
double star worked by hand, and redundancy.py's per-message helpers on
hand-computed arrays.

fresh_curve_ref evaluates the first-receipt formula on the C oracle's matrix.
The replay below shares nothing with it but the crash draw: it walks the rounds
with frontiers as sets and every arc, and books an arrival under (receipt
round, message) when the receiver is up and does not hold the message at the
start of the round -- several neighbours delivering one message in one round
all count.
"""
import numpy as np
import pytest

import directed_shapes as ds
import fresh_curve_ref
import fresh_ref


def replay(g, origin, inject, crashed_at, max_rounds=254):
    n, m = int(g.n), len(origin)
    outs = [[] for _ in range(n)]
    for v in range(n):
        for u in g.col[g.row_ptr[v]:g.row_ptr[v + 1]].tolist():
            outs[u].append(v)
    held = [set() for _ in range(n)]
    frontier = [set() for _ in range(n)]
    rows = [[0] * m]
    per_round = []
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
        row = [0] * m
        for u in range(n):
            for k in frontier[u]:
                for w in outs[u]:
                    if up[w] and k not in before[w]:
                        row[k] += 1
                        nxt[w].add(k)
        new = 0
        for w in range(n):
            held[w] |= nxt[w]
            new += len(nxt[w])
        frontier = nxt
        rows.append(row)
        per_round.append(np.array(rows, np.int64))
        if new == 0 and r >= last:
            break
    return per_round


def identities(g, origin, inject, ref, exp, fresh):
    """the consequences DESIGN.md §2.4 lists"""
    fc = exp["curve"]
    first = ref["first"]
    R, m = ref["rounds"], first.shape[1]
    assert fc.shape == (R + 1, m) and not fc[0].any() and (fc >= 0).all()
    # row sums: the growth of sum fresh_recv, round by round
    prev = 0
    for r, (_, rv) in enumerate(fresh["per_round"]):
        assert int(fc[r + 1].sum()) == int(rv.sum()) - prev, r
        prev = int(rv.sum())
    assert int(fc.sum()) == int(fresh["recv"].sum()) == int(fresh["sent"].sum())
    # lower bound: every expansion receipt has at least one deliverer
    hist = np.stack([(first == r).sum(axis=0) for r in range(R + 1)]).astype(np.int64)
    injected = np.zeros((R + 1, m), np.int64)
    up_origin = first[origin, np.arange(m)] != 255           # (a message lost at a down origin never existed)
    injected[inject[up_origin], np.nonzero(up_origin)[0]] = 1
    assert (fc[1:] >= (hist - injected)[1:]).all()
    assert (fc.sum(axis=0) >= np.maximum(ref["coverage"].astype(np.int64) - 1, 0)).all()
    # upper bound: no more deliveries than sends
    for r in range(R):
        assert int(fc[r + 1].sum()) <= ref["stats"][r]["sends"], r
    if ref["forwards"] is not None:
        assert (fc.sum(axis=0) <= ref["forwards"].astype(np.int64)).all()


def check(oracle, g, origin, inject, crashes=(), **churn):
    ref = oracle.run(g, origin, inject, crashes=crashes, want_first=True, **churn)
    exp = fresh_curve_ref.curve(g, ref, crashes=crashes, **churn)
    got = replay(g, origin.tolist(), inject.tolist(), exp["crashed_at"].tolist())
    assert len(got) == ref["rounds"] == len(exp["per_round"])
    for r, (a, b) in enumerate(zip(got, exp["per_round"])):
        assert a.shape == b.shape == (r + 2, len(origin))
        assert np.array_equal(a, b), (r, np.argwhere(a != b)[:8])
    assert np.array_equal(exp["curve"], got[-1])
    cut = fresh_curve_ref.curve(g, ref, crashes=crashes, rounds=2, **churn)
    assert np.array_equal(cut["curve"], got[1])
    identities(g, origin, inject, ref, exp, fresh_ref.totals(g, ref, crashes=crashes, **churn))
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
    assert int(exp["curve"].sum()) > sum(s["new_bits"] for s in ref["stats"]) > 0   # some message came twice at once


def test_more_than_one_word(pkg, oracle):
    g = undirected(pkg, oracle, 120)
    origin, inject = messages(pkg, g, 150, 6)
    ref, exp = check(oracle, g, origin, inject)
    sample = fresh_curve_ref.curve(g, ref, words=[1])          # a big shape's sample of words
    assert sample["columns"].tolist() == list(range(64, 128))
    assert np.array_equal(sample["curve"], exp["curve"][:, 64:128])
    with pytest.raises(ValueError):
        fresh_curve_ref.curve(g, ref, words=[2])                # messages 128 .. 191: past the 150th


def test_two_deliverers_in_one_round_both_count(pkg, oracle):
    """a 4-cycle: the vertex opposite the origin gets the message from both of
    its neighbours in the same round"""
    rp = np.array([0, 2, 4, 6, 8], np.int64)
    col = np.array([1, 3, 0, 2, 1, 3, 0, 2], np.int32)
    g = pkg.CSR(4, rp, col, False)
    ref, exp = check(oracle, g, np.array([0], np.int32), np.array([0], np.int32))
    assert exp["curve"][:, 0].tolist() == [0, 2, 2, 0]


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
    assert not exp["curve"][:, 3].any()                           # lost at its down origin: nobody delivered it


@pytest.mark.parametrize("directed", [False, True])
def test_churn(pkg, oracle, directed):
    g = ds.oriented_chung_lu(pkg, oracle, 200, 8, 2.2, 5, "coin") if directed else undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 4)
    ref, exp = check(oracle, g, origin, inject, churn=True, p_fail=0.05, churn_seed=11)
    assert sum(s["crashed"] for s in ref["stats"]) > 0 and sum(s["removals"] for s in ref["stats"]) > 0


# -- the double star, by hand ---------------------------------------------------

def test_double_star_by_hand(pkg, oracle):
    L = 5000
    g = fresh_curve_ref.double_star(pkg, L)
    origin = np.array([0, 2, 1], np.int32)
    ref = oracle.run(g, origin, None, want_first=True)
    assert ref["rounds"] == 3 and ref["coverage"].tolist() == [L + 2] * 3
    exp = fresh_curve_ref.curve(g, ref)
    assert exp["curve"].tolist() == [[0, 0, 0], [5000, 2, 5000], [5000, 9998, 5000], [0, 0, 0]]
    assert np.array_equal(exp["curve"], fresh_curve_ref.double_star_expected(L, [False, True, False]))
    assert max(exp["live_arcs"]) >= 2 * L - 2
    identities(g, origin, np.zeros(3, np.int64), ref, exp, fresh_ref.totals(g, ref))


# -- redundancy.py's per-message helpers ----------------------------------------

FC = np.array([[0, 0, 0, 0], [3, 2, 0, 0], [5, 4, 0, 0], [0, 6, 0, 0]], np.uint64)
CV = np.array([[1, 1, 1, 0], [3, 2, 0, 0], [2, 2, 0, 0], [0, 3, 0, 0]], np.uint64)   # message 2: nobody else; 3: lost


def test_message_deliverers(pkg):
    red = pkg.redundancy
    d = red.message_deliverers(FC)
    assert d.dtype == np.int64 and d.tolist() == [8, 12, 0, 0]
    assert red.message_deliverers(np.zeros((1, 3), np.uint64)).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        red.message_deliverers(FC[1])                 # not [rounds + 1, m]
    with pytest.raises(ValueError):
        red.message_deliverers(FC[1:])                # row 0 must be zero


def test_deliverers_per_receipt(pkg):
    red = pkg.redundancy
    cov = CV.sum(axis=0)
    assert cov.tolist() == [6, 8, 1, 0]
    x = red.deliverers_per_receipt(FC, cov)
    assert x.dtype == np.float64 and x.tolist() == [8 / 5, 12 / 7, 0.0, 0.0]
    with pytest.raises(ValueError):
        red.deliverers_per_receipt(FC, cov[:3])
    with pytest.raises(ValueError):
        red.deliverers_per_receipt(FC, np.array([10, 8, 1, 0]))   # 9 receipts from 8 deliveries
    with pytest.raises(ValueError):
        red.deliverers_per_receipt(FC, np.array([6, 1, 1, 0]))    # 12 deliveries of a message nobody else received


def test_message_redundancy(pkg):
    red = pkg.redundancy
    x = red.message_redundancy(np.array([20, 7, 3, 0], np.uint64), np.array([6, 8, 1, 0], np.uint64))
    assert x.dtype == np.float64 and x.tolist() == [3.0, 0.0, 0.0, 0.0]   # 20 sends for 5 receipts; a tree; none
    # the per-message form of relative_redundancy
    assert x[0] == red.relative_redundancy(np.array([20]), 5)
    with pytest.raises(ValueError):
        red.message_redundancy(np.array([20, 7]), np.array([6, 8, 1]))
    with pytest.raises(ValueError):
        red.message_redundancy(np.array([4]), np.array([6]))          # 5 receipts from 4 sends
    with pytest.raises(ValueError):
        red.message_redundancy(np.zeros((2, 2)), np.zeros((2, 2)))


def test_deliverers_by_round(pkg):
    red = pkg.redundancy
    x = red.deliverers_by_round(FC, CV)
    assert x.dtype == np.float64 and x.shape == FC.shape
    assert x.tolist() == [[0, 0, 0, 0], [1.0, 1.0, 0, 0], [2.5, 2.0, 0, 0], [0, 2.0, 0, 0]]
    with pytest.raises(ValueError):
        red.deliverers_by_round(FC, CV[:3])
    with pytest.raises(ValueError):
        red.deliverers_by_round(FC[:, 0], CV[:, 0])
    bad = CV.copy()
    bad[2, 0] = 7                                     # 7 receipts, 5 deliverers and one injection at most
    with pytest.raises(ValueError):
        red.deliverers_by_round(FC, bad)
    bad = CV.copy()
    bad[3, 1] = 0                                     # deliveries without a receipt
    with pytest.raises(ValueError):
        red.deliverers_by_round(FC, bad)
