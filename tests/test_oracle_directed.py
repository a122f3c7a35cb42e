"""The C oracle on directed overlays with hubs: pinned to the per-peer harness
(its directed path transposes the in-CSR and walks the out-CSR), its own
invariants recomputed in numpy, and the preconditions of the shapes that
test_gpu_directed.py runs on the GPU -- checked here, where no GPU is needed,
so that a changed generator cannot leave a GPU case exercising nothing."""
import numpy as np
import pytest

import directed_shapes as ds
from test_oracle import _both

M = 130
SMALL = [("coin", 1500), ("down", 1500), ("up", 1500), ("first3", 800)]


def _small(pkg, oracle, kind, n):
    if kind == "first3":
        return ds.first3(pkg, n)
    return ds.oriented_chung_lu(pkg, oracle, n, 8, 2.3, 5, kind)


def _messages(pkg, g):
    """130 random origins, inject rounds k % 4; message 1 starts at a vertex
    without out-arcs."""
    origin = pkg.overlay.random_origins(g.n, M, 5).copy()
    sinks = np.nonzero(g.out_degree() == 0)[0]
    assert sinks.size
    origin[1] = sinks[0]
    return origin, (np.arange(M) % 4).astype(np.int32)


def _liveness(g, origin, run):
    if run == "plain":
        return {}
    if run == "churn":
        return dict(churn=True, p_fail=0.03, churn_seed=5)
    return dict(crashes=[(int(np.argmax(g.in_degree())), 1), (int(np.argmax(g.out_degree())), 2), (int(origin[0]), 0)])


@pytest.mark.parametrize("run", ["plain", "churn", "crashes"])
@pytest.mark.parametrize("kind,n", SMALL, ids=[k for k, _ in SMALL])
def test_oracle_equals_harness_directed(pkg, oracle, harness, kind, n, run):
    g = _small(pkg, oracle, kind, n)
    assert g.directed and not np.array_equal(g.in_degree(), g.out_degree())
    origin, inject = _messages(pkg, g)
    ref = _both(pkg, oracle, harness, g, origin, inject, **_liveness(g, origin, run))
    if run != "plain":
        assert sum(s["removals"] for s in ref["stats"]) > 0
        assert sum(s["reports"] for s in ref["stats"]) > 0


@pytest.mark.parametrize("kind,n", SMALL, ids=[k for k, _ in SMALL])
def test_sends_are_out_degree_times_frontier(pkg, oracle, kind, n):
    """Without liveness a vertex forwards in round r what it first held at
    round r, once, on every out-arc (Peer.py:402): sends and forwards follow
    from the first-receipt matrix and the out-degrees alone."""
    g = _small(pkg, oracle, kind, n)
    origin, inject = _messages(pkg, g)
    ref = oracle.run(g, origin, inject, want_first=True)
    dout = g.out_degree()
    first = ref["first"]
    for r, s in enumerate(ref["stats"]):
        fresh = first == r
        assert s["sends"] == int((fresh.sum(axis=1) * dout).sum()), r
        assert s["active"] == int((fresh.any(axis=1)).sum()), r
    held = first != 255
    assert np.array_equal(ref["forwards"], (held * dout[:, None]).sum(axis=0).astype(np.uint64))
    assert np.array_equal(ref["coverage"], held.sum(axis=0).astype(np.uint64))


@pytest.mark.parametrize("kind,n", SMALL, ids=[k for k, _ in SMALL])
def test_message_of_a_sink_stays_there(pkg, oracle, kind, n):
    g = _small(pkg, oracle, kind, n)
    origin, inject = _messages(pkg, g)
    ref = oracle.run(g, origin, inject)
    dout = g.out_degree()
    sinks = [k for k in range(M) if dout[origin[k]] == 0]
    assert 1 in sinks
    for k in sinks:
        assert ref["coverage"][k] == 1 and ref["forwards"][k] == 0


# -- preconditions of the GPU shapes ---------------------------------------

def test_coin_shape(pkg, oracle):
    g = ds.oriented_chung_lu(pkg, oracle, 30_000, 12, 2.1, 17, "coin")
    din, dout = g.in_degree(), g.out_degree()
    big = din + dout > 2048
    # candidates that cross DET_BIG only through their out-list
    assert int((big & (din <= 2048)).sum()) >= 3
    top = np.argsort(-(din + dout), kind="stable")[:6]
    assert big[top].all() and int((din[top] <= 2048).sum()) >= 3
    assert int((dout > 512).sum()) >= 4 and int((din > 64).sum()) >= 100
    assert (din == 0).any() and (dout == 0).any()
    assert int(((din >= 128) != (dout >= 128)).sum()) > 0   # split filter and pushed arcs disagree


def test_one_way_hub_shapes(pkg, oracle):
    down = ds.oriented_chung_lu(pkg, oracle, 20_000, 8, 2.2, 11, "down")
    up = ds.oriented_chung_lu(pkg, oracle, 20_000, 8, 2.2, 11, "up")
    assert int((down.out_degree() > 512).sum()) >= 4 and down.in_degree().max() <= 64
    assert int((up.in_degree() > 64).sum()) >= 100 and up.out_degree().max() <= 64
    assert (up.in_degree() == 0).any() and (down.out_degree() == 0).any()
    assert down.nnz == up.nnz   # one arc per undirected edge, opposite ways


def test_first3_at_scale_shape(pkg, oracle):
    g = ds.first3(pkg, 3000)
    din, dout = g.in_degree(), g.out_degree()
    assert din[:3].tolist() == [2999, 2998, 2997] and dout[:3].tolist() == [0, 1, 2]
    assert not din[3:].any() and (dout[3:] == 3).all()
    # the GPU case's two crash schedules: the run ends with round 3, a crash at
    # round r is detected at r + 2
    origin = pkg.overlay.random_origins(g.n, 300, seed=3)
    inject = (np.arange(300) % 4).astype(np.int32)
    kw = dict(churn=True, p_fail=0.02, churn_seed=3)
    late = oracle.run(g, origin, inject, crashes=[(0, 1), (1, 2), (2, 3)], **kw)
    assert late["rounds"] == 4 and {d for d, _, _ in late["reports"].tolist()} & {0, 1, 2} == {0}
    assert 2048 < late["n_reports"] < 2 * 2048
    early = oracle.run(g, origin, inject, crashes=[(0, 0), (1, 1), (2, 1)], **kw)
    assert early["rounds"] == 4 and {d for d, _, _ in early["reports"].tolist()} >= {0, 1, 2}
    assert early["n_reports"] > 2 * 2048


@pytest.mark.parametrize("schedule", ["round0", "spread"])
def test_two_tier_structure(pkg, oracle, schedule):
    g, A, B = ds.two_tier(pkg, oracle)
    din, dout = g.in_degree(), g.out_degree()
    assert 3 * A.size < g.n
    assert int((dout > 512).sum()) >= 4 and int((din + dout > 2048).sum()) >= 4
    assert int((din != dout).sum()) > 1000
    # cross arcs run from A's giant into B's giant only
    src, dst = g.arcs()
    cross = (src < 12_000) != (dst < 12_000)
    assert cross.sum() > 0 and (src[cross] < 12_000).all()
    assert np.isin(src[cross], A).all() and np.isin(dst[cross], B).all()
    m = 4096
    origin = ds.two_tier_origins(g, A, B, m, 7)
    mA, mB = ds.two_tier_counts(origin, A, B)
    assert mA == m // 3 and mA + mB == m - m // 64
    inject = None if schedule == "round0" else (np.arange(m) % 3).astype(np.int32)
    ref = ds.CachedOracle(oracle).run(g, origin, inject)
    row_a, row_b = ds.two_tier_masks(origin, A, B, 64)
    assert (ref["seen"][A] == row_a).all()    # exactly the A-giant messages, never more
    assert (ref["seen"][B] == row_b).all()    # all of both giants': complete
    held = ds.held_before_round(ref)
    assert (held * 2 >= g.n * m).any()
    # what is never held keeps the thin-round condition of narrow rows out of reach
    assert ((g.n * m - held) * 16 >= g.n * m).all()
