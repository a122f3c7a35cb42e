"""The expected delivery multiplicity of tests/mult_ref.py against a
per-delivery replay (CPU), and the identities DESIGN.md §2.4 states for it.

mult_ref evaluates the first-receipt formula on the C oracle's matrix.  The
replay below shares nothing with it but the crash draw: it walks the rounds of
§2.2 with frontiers as sets and every arc, and for every first receipt keeps the
list of the peers whose line delivered it in that round -- parallel arcs and
all.  Overlays of at most 200 vertices: undirected, directed, with parallel
arcs, with explicit crashes and with churn.
"""
import numpy as np
import pytest

import directed_shapes as ds
import fresh_ref
import mult_ref


def replay(g, origin, inject, crashed_at, max_rounds=254):
    n, m = int(g.n), len(origin)
    outs = [[] for _ in range(n)]
    for v in range(n):
        for u in g.col[g.row_ptr[v]:g.row_ptr[v + 1]].tolist():
            outs[u].append(v)                 # (a parallel arc: twice)
    held = [set() for _ in range(n)]
    frontier = [set() for _ in range(n)]
    hist = [0] * 17
    sole_recv, sole_sent = [0] * n, [0] * n
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
                hist[0] += 1                  # a receipt nobody delivered
        before = [set(h) for h in held]      # what every peer holds at the start of E_r
        by = {}                               # (receiver, message) -> the deliverers, one entry per line
        for u in range(n):
            for k in frontier[u]:
                for w in outs[u]:
                    if up[w] and k not in before[w]:
                        by.setdefault((w, k), []).append(u)
        nxt = [set() for _ in range(n)]
        for (w, k), who in by.items():
            nxt[w].add(k)
            hist[min(len(who), 16)] += 1
            if len(who) == 1:
                sole_recv[w] += 1
                sole_sent[who[0]] += 1
        for w in range(n):
            held[w] |= nxt[w]
        frontier = nxt
        news.append(len(by))
        per_round.append((np.array(hist, np.int64), np.array(sole_recv, np.int64), np.array(sole_sent, np.int64)))
        if not by and r >= last:
            break
    return per_round, news


def check(oracle, g, origin, inject, crashes=(), **churn):
    ref = oracle.run(g, origin, inject, crashes=crashes, want_first=True, **churn)
    exp = mult_ref.totals(g, ref, crashes=crashes, **churn)
    got, news = replay(g, origin.tolist(), inject.tolist(), exp["crashed_at"].tolist())
    assert len(got) == ref["rounds"] == len(exp["per_round"])
    assert news == [s["new_bits"] for s in ref["stats"]]
    for r, (a, b) in enumerate(zip(got, exp["per_round"])):
        for x, y, name in zip(a, b, ("hist", "sole_recv", "sole_sent")):
            assert np.array_equal(x, y), (r, name, np.nonzero(x != y)[0][:8])
    for x, y in zip(got[-1], (exp["hist"], exp["sole_recv"], exp["sole_sent"])):
        assert np.array_equal(x, y)
    cut = mult_ref.totals(g, ref, crashes=crashes, rounds=2, **churn)
    for x, y in zip(got[1], (cut["hist"], cut["sole_recv"], cut["sole_sent"])):
        assert np.array_equal(x, y)
    identities(g, origin, ref, exp, fresh_ref.totals(g, ref, crashes=crashes, **churn))
    return ref, exp


def identities(g, origin, ref, exp, fresh):
    """the consequences DESIGN.md §2.4 lists"""
    hist = exp["hist"]
    assert int(hist.sum()) == int(ref["coverage"].sum())
    assert int(hist[1:].sum()) == sum(s["new_bits"] for s in ref["stats"])
    assert int(hist[0]) == sum(s["injected"] for s in ref["stats"])
    assert int(hist[1]) == int(exp["sole_recv"].sum()) == int(exp["sole_sent"].sum())
    first = ref["first"]
    m = first.shape[1]
    injected = first[origin, np.arange(m)] != 255          # (a message lost at a down origin never existed)
    own = np.bincount(origin[injected], minlength=g.n)
    assert (exp["sole_recv"] <= (first != 255).sum(axis=1) - own).all()
    assert (exp["sole_recv"] <= fresh["recv"]).all() and (exp["sole_sent"] <= fresh["sent"]).all()
    weighted = sum(c * int(hist[c]) for c in range(1, 17))
    assert weighted <= int(fresh["recv"].sum())
    if hist[16] == 0:
        assert weighted == int(fresh["recv"].sum())        # nothing saturated: the mean is fresh / receipts
    for r, (h, sr, ss) in enumerate(exp["per_round"]):
        assert int(h[1:].sum()) == sum(s["new_bits"] for s in ref["stats"][:r + 1]), r
        assert int(h[0]) == sum(s["injected"] for s in ref["stats"][:r + 1]), r
        assert int(h[1]) == int(sr.sum()) == int(ss.sum())


def messages(pkg, g, m, seed):
    return pkg.overlay.random_origins(g.n, m, seed=seed), (np.arange(m) % 4).astype(np.int32)


def undirected(pkg, oracle, n=200):
    rp, col = oracle.chung_lu(n, 4, 2.2, 3)
    return pkg.CSR(n, rp, col, False)


def test_undirected_nobody_down(pkg, oracle):
    g = undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 1)
    ref, exp = check(oracle, g, origin, inject)
    assert exp["hist"][1] > 0 and exp["hist"][2:].sum() > 0     # sole and shared receipts both occur


def test_path_every_receipt_is_sole(pkg, oracle):
    """a path: every message reaches every peer from one neighbour only"""
    n = 9
    rp = np.array([0] + [1 if v in (0, n - 1) else 2 for v in range(n)], np.int64).cumsum()
    col = np.array([u for v in range(n) for u in (v - 1, v + 1) if 0 <= u < n], np.int32)
    g = pkg.CSR(n, rp, col, False)
    origin, inject = np.array([0, 4, 8], np.int32), np.array([0, 1, 0], np.int32)
    ref, exp = check(oracle, g, origin, inject)
    assert exp["hist"].tolist() == [3, 3 * (n - 1)] + [0] * 15
    own = np.bincount(origin, minlength=n)
    assert np.array_equal(exp["sole_recv"], (ref["first"] != 255).sum(axis=1) - own)


def test_four_cycle_two_deliverers(pkg, oracle):
    """a 4-cycle: the vertex opposite the origin gets the message from both of
    its neighbours in the same round -- no sole deliverer for that receipt"""
    rp = np.array([0, 2, 4, 6, 8], np.int64)
    col = np.array([1, 3, 0, 2, 1, 3, 0, 2], np.int32)
    g = pkg.CSR(4, rp, col, False)
    ref, exp = check(oracle, g, np.array([0], np.int32), np.array([0], np.int32))
    assert exp["hist"].tolist() == [1, 2, 1] + [0] * 14
    assert exp["sole_recv"].tolist() == [0, 1, 0, 1] and exp["sole_sent"].tolist() == [2, 0, 0, 0]


def test_star_saturates(pkg, oracle):
    """20 leaves that all hold the message deliver it to the centre of a second
    star in one round: 16 or more is one bin, and 15 is not in it"""
    def two_level(k):
        # origin 0 -> k middle peers -> sink k + 1 (directed)
        n = k + 2
        ins = [[] for _ in range(n)]
        for u in range(1, k + 1):
            ins[u].append(0)
            ins[n - 1].append(u)
        rp = np.cumsum([0] + [len(x) for x in ins]).astype(np.int64)
        col = np.array([u for x in ins for u in x], np.int32)
        return pkg.CSR(n, rp, col, True)
    for k, b in ((15, 15), (16, 16), (20, 16), (40, 16)):
        g = two_level(k)
        ref, exp = check(oracle, g, np.array([0], np.int32), np.array([0], np.int32))
        want = [0] * 17
        want[0] = 1
        want[1] = k
        want[b] += 1
        assert exp["hist"].tolist() == want, k
        assert exp["sole_sent"][0] == k and exp["sole_recv"][k + 1] == 0


def test_parallel_arcs_count_separately(pkg, oracle):
    """0 -> 1 twice: the receipt at 1 has two deliverers (no sole one); 1 -> 2
    once: sole"""
    rp = np.array([0, 0, 2, 3], np.int64)
    col = np.array([0, 0, 1], np.int32)
    g = pkg.CSR(3, rp, col, True)
    ref, exp = check(oracle, g, np.array([0, 0], np.int32), np.array([0, 1], np.int32))
    assert exp["hist"].tolist() == [2, 2, 2] + [0] * 14
    assert exp["sole_sent"].tolist() == [0, 2, 0] and exp["sole_recv"].tolist() == [0, 0, 2]
    # ... and on a random overlay with some arcs doubled
    g0 = undirected(pkg, oracle, 120)
    ins = [g0.col[g0.row_ptr[v]:g0.row_ptr[v + 1]].tolist() for v in range(g0.n)]
    rng = np.random.default_rng(6)
    for v in range(g0.n):
        ins[v] += [u for u in ins[v] if rng.random() < 0.3]
    rp = np.cumsum([0] + [len(x) for x in ins]).astype(np.int64)
    g = pkg.CSR(g0.n, rp, np.array([u for x in ins for u in x], np.int32), True)
    origin, inject = messages(pkg, g, 64, 5)
    check(oracle, g, origin, inject)


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
    # a vertex that crashed in the round it would have sent was nobody's sole deliverer for that receipt
    plain_exp = mult_ref.totals(g, plain)
    assert int(exp["sole_sent"][got2].sum()) <= int(plain_exp["sole_sent"][got2].sum())
    assert not np.array_equal(exp["hist"], plain_exp["hist"])


@pytest.mark.parametrize("directed", [False, True])
def test_churn(pkg, oracle, directed):
    g = ds.oriented_chung_lu(pkg, oracle, 200, 8, 2.2, 5, "coin") if directed else undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 4)
    ref, exp = check(oracle, g, origin, inject, churn=True, p_fail=0.05, churn_seed=11)
    assert sum(s["crashed"] for s in ref["stats"]) > 0 and sum(s["removals"] for s in ref["stats"]) > 0


def test_chunk_report(pkg, oracle):
    """the hub test's precondition figures on a shape small enough to brute-force:
    big_hist and cross against a direct count over the in-lists"""
    g = undirected(pkg, oracle)
    origin, inject = messages(pkg, g, 70, 1)
    ref = oracle.run(g, origin, inject, want_first=True)
    C = 4
    exp = mult_ref.totals(g, ref, chunk=C)
    first = ref["first"]
    big_hist, cross = [0] * 17, 0
    for v in range(g.n):
        ins = g.col[g.row_ptr[v]:g.row_ptr[v + 1]].tolist()
        if len(ins) <= C:
            continue
        for k in range(first.shape[1]):
            if first[v][k] in (0, 255):
                continue
            at = [p for p, u in enumerate(ins) if first[u][k] != 255 and first[u][k] + 1 == first[v][k]]
            if not at:
                continue
            big_hist[min(len(at), 16)] += 1
            if 2 <= len(at) <= 15 and len({p // C for p in at}) > 1:
                cross += 1
    assert exp["big_hist"].tolist() == big_hist and exp["cross"] == cross > 0
