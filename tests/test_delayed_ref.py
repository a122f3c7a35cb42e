"""tests/delayed_ref.py, the numpy reference of the delayed-link semantics
(DESIGN.md §2.2), pinned on the CPU: with dmax = 1 it is the C oracle's flood
and, under loss, lossy_ref.run; with dmax > 1 its first receipts are the
shortest paths under the delays, and on a path they follow from the delays
alone."""
import functools

import numpy as np
import pytest

import delayed_ref
import directed_shapes as ds
import lossy_ref

FLOOD_KEYS = ("injected", "new_bits", "receivers", "sends", "active")


@functools.lru_cache(maxsize=None)
def _case(pkg, oracle, directed):
    if directed:
        g = ds.oriented_chung_lu(pkg, oracle, 4099, 8, 2.2, 7, "coin")
    else:
        rp, col = oracle.chung_lu(4099, 8, 2.2, 7)
        g = pkg.CSR(4099, rp, col, False)
    origin = pkg.overlay.random_origins(g.n, 100, seed=100)
    inject = (np.arange(100) % 3).astype(np.int32)
    return g, origin, inject, oracle.run(g, origin, inject, want_first=True)


def _same_run(got, ref):
    assert got["rounds"] == ref["rounds"]
    assert np.array_equal(got["first"], ref["first"])
    for a, b in zip(got["stats"], ref["stats"]):
        for k in FLOOD_KEYS:
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    assert np.array_equal(got["coverage"], ref["coverage"])
    assert np.array_equal(got["forwards"], ref["forwards"])


@pytest.mark.parametrize("directed", [False, True], ids=["chung-lu", "oriented"])
def test_one_round_links_are_the_oracles_flood(pkg, oracle, directed):
    g, origin, inject, ref = _case(pkg, oracle, directed)
    got = delayed_ref.run(g, origin, inject, dmax=1, seed=3)
    _same_run(got, ref)
    assert got["by_delay"][1] == sum(s["new_bits"] for s in ref["stats"])
    if not directed:
        assert ref["rounds"] >= 8


def test_one_round_links_with_loss_are_lossy_ref(pkg, oracle):
    g, origin, inject, ref = _case(pkg, oracle, False)
    want = lossy_ref.run(g, origin, inject, p=0.5, seed=11)
    assert not np.array_equal(want["first"], ref["first"])
    _same_run(delayed_ref.run(g, origin, inject, dmax=1, seed=3, p=0.5, loss_seed=11), want)


def _dist(g, delay, origin):
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import dijkstra
    except ImportError:
        return delayed_ref.shortest(g, delay, origin)
    n = int(g.n)
    rp = np.asarray(g.row_ptr, np.int64)
    src = np.asarray(g.col, np.int64)
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    # (parallel arcs share their delay: keep one of each, csr_matrix would add them)
    pair, keep = np.unique(src * n + dst, return_index=True)
    w = csr_matrix((np.asarray(delay, np.float64)[keep], (pair // n, pair % n)), shape=(n, n))
    uniq, inv = np.unique(np.asarray(origin, np.int64), return_inverse=True)
    d = dijkstra(w, directed=True, indices=uniq)          # [origins][n]
    d = np.where(np.isinf(d), float(1 << 40), d).astype(np.int64)
    return d.T[:, inv]


@pytest.mark.parametrize("directed", [False, True], ids=["chung-lu", "oriented"])
@pytest.mark.parametrize("dmax", [2, 4, 8])
def test_first_receipts_are_shortest_paths(pkg, oracle, dmax, directed):
    g, origin, inject, ref = _case(pkg, oracle, directed)
    got = delayed_ref.run(g, origin, inject, dmax=dmax, seed=11)
    delay = delayed_ref.arc_delays(g, dmax, 11)
    assert delay.min() == 1 and delay.max() == dmax
    dist = _dist(g, delay, origin)
    want = np.where(dist < (1 << 40), dist + inject[None, :], 255)
    assert want[want != 255].max() < 255
    assert np.array_equal(got["first"], want.astype(np.uint8))
    assert np.array_equal(got["coverage"], ref["coverage"])
    assert got["rounds"] > ref["rounds"] and (got["by_delay"][1:] > 0).all()
    share = float((got["first"] != ref["first"]).mean())
    print(f"dmax={dmax} directed={directed}: {share:.3f} of the cells differ from the flood's, {got['rounds']} rounds")
    if not directed:   # (the oriented overlay leaves many cells unreached in both runs)
        assert share >= 0.5
    # attempted sends, in the send round: the flood's per message
    assert np.array_equal(got["forwards"], ref["forwards"])
    assert sum(s["sends"] for s in got["stats"]) == sum(s["sends"] for s in ref["stats"])


def test_bellman_ford_is_dijkstra(pkg, oracle):
    """the numpy fallback of the shortest-path check against scipy's, where importable"""
    pytest.importorskip("scipy")
    g, origin, inject, ref = _case(pkg, oracle, True)
    delay = delayed_ref.arc_delays(g, 4, 11)
    assert np.array_equal(delayed_ref.shortest(g, delay, origin[:10]), _dist(g, delay, origin[:10]))


def path_case(pkg, n=6, dmax=4):
    """a path 0 - 1 - ... - n-1, one message at vertex 0, and the first seed
    whose path holds a delay > 1 (asserted on the twin alone)"""
    i = np.arange(n - 1)
    g = pkg.CSR.from_arcs(n, np.concatenate([i, i + 1]), np.concatenate([i + 1, i]), directed=False)
    for seed in range(64):
        d = pkg.lag.arc_delay(seed, i, i + 1, dmax).astype(np.int64)
        if d.max() > 1:
            break
    assert d.max() > 1 and d.min() >= 1
    return g, np.zeros(1, np.int32), np.zeros(1, np.int32), seed, d


def test_path_follows_from_the_delays(pkg):
    g, origin, inject, seed, d = path_case(pkg)
    got = delayed_ref.run(g, origin, inject, dmax=4, seed=seed)
    want = np.concatenate([[0], np.cumsum(d)])
    assert np.array_equal(got["first"][:, 0].astype(np.int64), want)
    # rounds without a new bit before the last receipt, and dmax rounds of draining after it
    quiet = [s["round"] for s in got["stats"] if s["new_bits"] == 0]
    assert quiet and min(quiet) + 1 < want[-1]
    assert got["rounds"] == int(d.sum()) + 4


@pytest.mark.parametrize("dmax", [2, 4])
def test_crashed_sender_lines_still_arrive(pkg, oracle, dmax):
    """a sender that crashes after its send round: its lines in flight arrive"""
    import load_ref
    g, origin, inject, ref = _case(pkg, oracle, False)
    plain = delayed_ref.run(g, origin, inject, dmax=dmax, seed=11)
    picked = np.nonzero((plain["first"] == 3).any(axis=1))[0][:20]
    assert picked.size == 20
    late = delayed_ref.run(g, origin, inject, dmax=dmax, seed=11,
                           crash_at=load_ref.crash_rounds(g.n, 64, [(int(v), 5) for v in picked]))
    early = delayed_ref.run(g, origin, inject, dmax=dmax, seed=11,
                            crash_at=load_ref.crash_rounds(g.n, 64, [(int(v), 3) for v in picked]))
    assert sum(s["crashed"] for s in late["stats"]) == 20 == sum(s["crashed"] for s in early["stats"])
    rp = np.asarray(g.row_ptr, np.int64)
    src = np.asarray(g.col, np.int64)
    dst = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(rp))
    delay = delayed_ref.arc_delays(g, dmax, 11)
    # crashed in round 5: what they sent in round 3 over a link of d >= 2 arrives in a round in which
    # they are down already, and it does arrive (at a receiver that is up)
    arcs = np.nonzero(np.isin(src, picked) & (delay >= 2) & ~np.isin(dst, picked))[0]
    assert arcs.size > 20
    checked = 0
    for j in arcs:
        ks = np.nonzero(late["first"][src[j]] == 3)[0]
        assert (late["first"][dst[j]][ks] <= 3 + delay[j]).all()
        checked += int((late["first"][dst[j]][ks] == 3 + delay[j]).sum())
    assert checked > 0   # (some of those lines were the first to arrive)
    # crashed in round 3, right after the receipt: the receipts up to round 3 are the plain run's, and
    # the picked peers are missing from round 3's senders
    assert np.array_equal(early["first"] <= 3, plain["first"] <= 3)
    deg = np.diff(rp)
    held = (plain["first"][picked] == 3)
    assert early["stats"][3]["active"] == plain["stats"][3]["active"] - 20
    assert early["stats"][3]["sends"] == plain["stats"][3]["sends"] - int((deg[picked] * held.sum(axis=1)).sum())
    assert not np.array_equal(early["first"], late["first"])
