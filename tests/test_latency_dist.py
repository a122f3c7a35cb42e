"""latency.py's readers of the per-peer delay distributions (pure numpy, CPU):
dist_quantile, dist_bins, dist_by_degree, dist_combine, dist_check -- on
hand-made rows whose answers are known, and every ValueError."""
import numpy as np
import pytest


def row(**cols):
    r = np.zeros(16, np.uint16)
    for k, v in cols.items():
        r[int(k[1:])] = v
    return r


def test_quantile_lower_value_rule(pkg):
    L = pkg.latency
    dist = np.stack([
        row(d1=1, d2=1, d3=1, d4=1),          # delays 1 2 3 4
        row(d0=1, d3=8, d7=1),                # 0, eight 3s, 7
        row(),                                # never reached
        row(d2=5, d15=5),                     # half of it saturated
        row(d15=3),                           # all saturated
        row(d5=10),                           # ten equal delays
    ])
    assert np.array_equal(L.dist_quantile(dist, 0.5), [2, 3, np.nan, 2, 15, 5], equal_nan=True)
    assert np.array_equal(L.dist_quantile(dist, 0.9), [4, 3, np.nan, 15, 15, 5], equal_nan=True)   # ceil(0.9 * 10) = 9, not 10
    assert np.array_equal(L.dist_quantile(dist, 1.0), [4, 7, np.nan, 15, 15, 5], equal_nan=True)
    assert np.array_equal(L.dist_quantile(dist, 0.0), [1, 0, np.nan, 2, 15, 5], equal_nan=True)    # the first receipt
    assert np.array_equal(L.dist_quantile(dist, 0.25), [1, 3, np.nan, 2, 15, 5], equal_nan=True)
    val, sat = L.dist_quantile(dist, 0.9, flag=True)
    assert sat.tolist() == [False, False, False, True, True, False]
    assert L.dist_quantile(dist, 0.5).dtype == np.float64
    # against the sorted delays, receipt by receipt
    rng = np.random.Generator(np.random.PCG64(5))
    big = rng.integers(0, 40, (50, 16)).astype(np.uint16)
    for q in (0.5, 0.9, 0.99, 0.1):
        got = L.dist_quantile(big, q)
        for v in range(50):
            delays = np.repeat(np.arange(16), big[v])
            rank = max(1, -(-int(round(q * 100)) * delays.size // 100))   # ceil(q * total), in integers
            assert got[v] == delays[rank - 1]


def test_quantile_errors(pkg):
    L = pkg.latency
    ok = np.zeros((3, 16), np.uint16)
    for bad in (np.zeros((3, 15), np.uint16), np.zeros(16, np.uint16), np.zeros((3, 16), np.float64),
                np.full((3, 16), -1, np.int64)):
        with pytest.raises(ValueError):
            L.dist_quantile(bad, 0.5)
    for q in (-0.1, 1.5):
        with pytest.raises(ValueError):
            L.dist_quantile(ok, q)
    assert np.isnan(L.dist_quantile(ok, 0.5)).all()
    assert L.dist_quantile(np.zeros((0, 16), np.uint16), 0.5).shape == (0,)


def test_bins_and_by_degree(pkg):
    L = pkg.latency
    deg = np.array([0, 1, 2, 3, 4, 900])
    dist = np.stack([row(), row(d3=2), row(d2=1, d3=1), row(d2=2), row(d1=4), row(d0=1, d1=9, d15=1)])
    t = L.dist_bins(deg, dist)
    assert t.dtype == np.uint64 and t.shape == (32, 16)
    assert t[0].tolist() == row(d3=2).tolist() and t[1].tolist() == row(d2=3, d3=1).tolist()
    assert t[2].tolist() == row(d1=4).tolist() and t[9].tolist() == row(d0=1, d1=9, d15=1).tolist()
    assert int(t.sum()) == int(dist.sum())
    rows = L.dist_by_degree(t)
    assert [r["bin"] for r in rows] == [0, 1, 2, 9]
    assert rows[0] == dict(bin=0, deg_lo=0, deg_hi=1, receipts=2, mean_delay=3.0, p50=3, p90=3, p99=3, saturated=False)
    assert rows[1]["p50"] == 2 and rows[1]["p90"] == 3 and (rows[1]["deg_lo"], rows[1]["deg_hi"]) == (2, 3)
    assert rows[3]["p50"] == 1 and rows[3]["p90"] == 1 and rows[3]["p99"] == 15 and rows[3]["saturated"]
    assert rows[3]["mean_delay"] == (9 + 15) / 11
    assert [set(r) >= {"p25"} for r in L.dist_by_degree(t, qs=(0.25,))] == [True] * 4
    with pytest.raises(ValueError):
        L.dist_bins(deg[:5], dist)              # degrees of another overlay
    with pytest.raises(ValueError):
        L.dist_bins(deg, dist[:, :15])
    with pytest.raises(ValueError):
        L.dist_bins(deg.astype(np.float64), dist)
    for bad in (np.zeros((32, 5), np.uint64), np.zeros((31, 16), np.uint64), np.zeros((32, 16), np.float64),
                np.full((32, 16), -1, np.int64)):
        with pytest.raises(ValueError):
            L.dist_by_degree(bad)


def test_combine(pkg):
    L = pkg.latency
    a = np.full((3, 16), 40000, np.uint16)
    out = L.dist_combine([a, a])
    assert out.dtype == np.int64 and (out == 80000).all()     # (past u16: added in a wider type)
    assert np.array_equal(L.dist_combine([a]), a.astype(np.int64))
    t = np.ones((32, 16), np.uint64)
    assert (L.dist_combine([t, t, t]) == 3).all()             # tables add the same way
    for bad in ([], [a, a[:2]], [a, a.astype(np.float32)], [a[:, :15]], [a[0]]):
        with pytest.raises(ValueError):
            L.dist_combine(bad)


def test_check(pkg):
    L = pkg.latency
    dist = np.stack([row(d0=1, d2=2, d5=1), row(), row(d14=1, d15=2), row(d15=1)])
    sp = np.array([4, 0, 3, 1], np.uint32)
    ds = np.array([9, 0, 14 + 15 + 40, 15], np.uint32)
    dm = np.array([5, 0, 40, 15], np.uint8)
    L.dist_check(dist, sp)
    L.dist_check(dist, sp, ds)
    L.dist_check(dist, sp, ds, dm)
    L.dist_check(dist, sp, delay_max=dm)

    def fails(*args, **kw):
        with pytest.raises(ValueError):
            L.dist_check(*args, **kw)

    fails(dist, sp + np.array([1, 0, 0, 0], np.uint32))                         # a row does not sum to seenpop
    fails(dist[:3], sp)                                                         # arrays of different runs
    fails(dist, sp, ds + np.array([1, 0, 0, 0], np.uint32))                     # exact where column 15 is empty
    fails(dist, sp, ds - np.array([1, 0, 0, 0], np.uint32))
    fails(dist, sp, ds - np.array([0, 0, 41, 0], np.uint32))                    # below the weighted sum
    L.dist_check(dist, sp, ds + np.array([0, 0, 500, 7], np.uint32))            # above it: the tail may be later
    fails(dist, sp, ds, dm + np.array([1, 0, 0, 0], np.uint8))                  # the largest occupied column
    fails(dist, sp, ds, np.array([5, 0, 14, 15], np.uint8))                     # saturated, delay_max < 15
    fails(dist, sp, ds[:3])
    fails(dist, sp, ds, dm[:3])
    fails(dist.astype(np.float64), sp)
    fails(dist, sp.astype(np.float64))
    fails(dist[:, :8], sp)
