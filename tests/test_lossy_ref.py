"""tests/lossy_ref.py, the numpy reference of the lossy-link semantics
(DESIGN.md §2.2), pinned on the CPU: with every arc open it is the C oracle's
flood, on a path its reaches follow from the draw alone, and with every arc
closed only the injections remain."""
import numpy as np
import pytest

import directed_shapes as ds
import lossy_ref

FLOOD_KEYS = ("injected", "new_bits", "receivers", "sends", "active")


def _flood_case(pkg, oracle, g, m):
    origin = pkg.overlay.random_origins(g.n, m, seed=m)
    inject = (np.arange(m) % 3).astype(np.int32)
    ref = oracle.run(g, origin, inject, want_first=True)
    got = lossy_ref.run(g, origin, inject, p=0.0, seed=3)
    assert got["rounds"] == ref["rounds"]
    assert np.array_equal(got["first"], ref["first"])
    for a, b in zip(got["stats"], ref["stats"]):
        for k in FLOOD_KEYS:
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    assert np.array_equal(got["coverage"], ref["coverage"])
    assert np.array_equal(got["forwards"], ref["forwards"])
    return ref


def test_every_arc_open_is_the_oracles_flood(pkg, oracle):
    rp, col = oracle.chung_lu(4099, 8, 2.2, 7)
    ref = _flood_case(pkg, oracle, pkg.CSR(4099, rp, col, False), 100)
    assert ref["rounds"] >= 8


def test_every_arc_open_directed(pkg, oracle):
    g = ds.oriented_chung_lu(pkg, oracle, 4099, 8, 2.2, 7, "coin")
    _flood_case(pkg, oracle, g, 100)


@pytest.mark.parametrize("seed", [5, 6])
def test_path_reaches_follow_from_the_draw(pkg, seed):
    """40-vertex path, 64 messages at vertex 0, inject = k % 5: message k goes
    0 -> 1 -> ... one hop per round, over arc (i, i + 1) in round inject + i, and
    stops for good at the first closed one"""
    n, m, p = 40, 64, 0.1
    i = np.arange(n - 1)
    g = pkg.CSR.from_arcs(n, np.concatenate([i, i + 1]), np.concatenate([i + 1, i]), directed=False)
    origin = np.zeros(m, np.int32)
    inject = (np.arange(m) % 5).astype(np.int32)
    got = lossy_ref.run(g, origin, inject, p=p, seed=seed)
    reach = np.zeros(m, np.int64)
    for k in range(m):
        d = 0
        while d < n - 1 and pkg.loss.arc_open(seed, int(inject[k]) + d, [d], [d + 1], p)[0]:
            d += 1
        reach[k] = d
        want = np.full(n, 255, np.uint8)
        want[:d + 1] = inject[k] + np.arange(d + 1)
        assert np.array_equal(got["first"][:, k], want), (k, d)
    assert len(set(reach.tolist())) >= 3 and reach.max() > reach.min()
    assert np.array_equal(got["coverage"], (reach + 1).astype(np.uint64))


def test_every_arc_closed_leaves_the_injections(pkg, oracle):
    rp, col = oracle.chung_lu(4099, 8, 2.2, 7)
    g = pkg.CSR(4099, rp, col, False)
    origin = pkg.overlay.random_origins(g.n, 100, seed=100)
    inject = (np.arange(100) % 3).astype(np.int32)
    got = lossy_ref.run(g, origin, inject, p=1.0, seed=1)
    assert got["rounds"] == 3 and all(s["new_bits"] == 0 for s in got["stats"])
    assert (got["coverage"] == 1).all()
    assert np.array_equal(got["first"][origin, np.arange(100)], inject.astype(np.uint8))
    assert sum(s["sends"] for s in got["stats"]) == int(np.diff(rp)[origin].sum())
