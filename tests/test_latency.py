"""latency.py, the helpers that read the per-peer receipt delays, on hand-made
arrays (CPU): mean delay with an unreached peer, the numpy twin of the device's
degree table with degree 0, the by-degree reading, and the two functions of the
spread curve that tie it to the record."""
import numpy as np
import pytest

# five peers: a leaf, a hub, an isolated vertex (degree 0, unreached), an origin
# that holds only its own message (delay 0), a degree-1 peer never reached
DEG = np.array([2, 9, 0, 3, 1])
SEENPOP = np.array([3, 3, 0, 1, 0], np.uint32)
DSUM = np.array([9, 4, 0, 0, 0], np.uint32)
DMAX = np.array([4, 2, 0, 0, 0], np.uint8)


def test_mean_delay(pkg):
    lat = pkg.latency
    mean = lat.mean_delay(DSUM, SEENPOP)
    assert mean.dtype == np.float64
    assert mean[:2].tolist() == [3.0, 4 / 3] and mean[3] == 0.0
    assert np.isnan(mean[2]) and np.isnan(mean[4])   # never reached: no mean, not 0
    assert lat.mean_delay(np.zeros(0, np.uint32), np.zeros(0, np.uint32)).size == 0


def test_degree_bin(pkg):
    lat = pkg.latency
    deg = [0, 1, 2, 3, 4, 7, 8, 913, 1023, 1024, 2 ** 31 - 1]
    assert lat.degree_bin(deg).tolist() == [0, 0, 1, 1, 2, 2, 3, 9, 9, 10, 30]
    assert lat.degree_bin(5).tolist() == [2]
    # exact at every power of two and one below it
    for k in range(1, 32):
        assert lat.degree_bin([(1 << k) - 1, 1 << k]).tolist() == [max(k - 1, 0) if k > 1 else 0, k]
    with pytest.raises(ValueError):
        lat.degree_bin([1 << 32])


def test_bins(pkg):
    lat = pkg.latency
    t = lat.bins(DEG, SEENPOP, DSUM, DMAX)
    assert t.dtype == np.uint64 and t.shape == (32, 5) == (lat.BINS, lat.COLS)
    assert t[0].tolist() == [2, 0, 0, 0, 0]       # degrees 0 and 1: neither reached
    assert t[1].tolist() == [2, 2, 4, 9, 4]       # degrees 2 and 3
    assert t[3].tolist() == [1, 1, 3, 4, 2]       # degree 9
    assert not t[[2] + list(range(4, 32))].any()
    assert int(t[:, 0].sum()) == DEG.size and int(t[:, 3].sum()) == int(DSUM.sum())
    empty = lat.bins(np.zeros(0, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8))
    assert empty.shape == (32, 5) and not empty.any()


def test_bins_refuse_arrays_of_different_runs(pkg):
    lat = pkg.latency
    with pytest.raises(ValueError):
        lat.bins(DEG[:4], SEENPOP, DSUM, DMAX)
    with pytest.raises(ValueError):   # a delay without a receipt
        lat.bins(DEG, np.array([3, 3, 0, 0, 0]), np.array([9, 4, 0, 1, 0]), DMAX)
    with pytest.raises(ValueError):   # the maximum exceeds the sum
        lat.bins(DEG, SEENPOP, DSUM, np.array([4, 5, 0, 0, 0]))
    with pytest.raises(ValueError):   # the sum exceeds seenpop * maximum
        lat.bins(DEG, SEENPOP, DSUM, np.array([2, 2, 0, 0, 0]))
    with pytest.raises(ValueError):
        lat.mean_delay(DSUM.astype(np.float64), SEENPOP)
    with pytest.raises(ValueError):
        lat.mean_delay(DSUM, SEENPOP[:3])


def test_by_degree(pkg):
    lat = pkg.latency
    rows = lat.by_degree(lat.bins(DEG, SEENPOP, DSUM, DMAX))
    assert [r["bin"] for r in rows] == [0, 1, 3]
    assert [(r["deg_lo"], r["deg_hi"]) for r in rows] == [(0, 1), (2, 3), (8, 15)]
    assert [r["peers"] for r in rows] == [2, 2, 1]
    assert [r["reach"] for r in rows] == [0.0, 1.0, 1.0]
    assert np.isnan(rows[0]["mean_delay"]) and rows[1]["mean_delay"] == 9 / 4 and rows[2]["mean_delay"] == 4 / 3
    assert [r["max_delay"] for r in rows] == [0, 4, 2]
    with pytest.raises(ValueError):
        lat.by_degree(np.zeros((31, 5), np.uint64))
    bad = lat.bins(DEG, SEENPOP, DSUM, DMAX)
    bad[1, 1] = 3   # more peers reached than peers
    with pytest.raises(ValueError):
        lat.by_degree(bad)


def test_combine(pkg):
    lat = pkg.latency
    whole = lat.bins(DEG, SEENPOP, DSUM, DMAX)
    parts = [lat.bins(DEG[a:b], SEENPOP[a:b], DSUM[a:b], DMAX[a:b]) for a, b in [(0, 2), (2, 3), (3, 5)]]
    assert np.array_equal(lat.combine(parts), whole)
    # two message shards of the same five peers
    s1 = lat.bins(DEG, [2, 1, 0, 1, 0], [5, 1, 0, 0, 0], [4, 1, 0, 0, 0])
    s2 = lat.bins(DEG, [1, 2, 0, 0, 0], [4, 3, 0, 0, 0], [4, 2, 0, 0, 0])
    both = lat.combine([s1, s2], disjoint=False)
    assert np.array_equal(both[:, [0, 2, 3, 4]], whole[:, [0, 2, 3, 4]]) and not both[:, 1].any()
    with pytest.raises(ValueError):
        lat.combine([])
    with pytest.raises(ValueError):
        lat.combine([s1, parts[0]], disjoint=False)


def test_delay_hist_and_total(pkg):
    lat = pkg.latency
    inject = np.array([0, 2, 1])
    curve = np.array([[1, 0, 0],     # receipt round 0: message 0's injection
                      [3, 0, 1],     # round 1: 3 receipts of message 0 (delay 1), message 2's injection
                      [5, 1, 2],     # round 2: delay 2, message 1's injection, delay 1
                      [0, 4, 0]], np.uint64)   # round 3: delay 1 of message 1
    hist = lat.delay_hist(curve, inject)
    assert hist.dtype == np.uint64 and hist.tolist() == [3, 3 + 2 + 4, 5, 0]
    assert int(hist.sum()) == int(curve.sum())
    assert lat.total_delay(curve, inject) == 3 * 1 + 5 * 2 + 2 * 1 + 4 * 1 == int((np.arange(4) * hist).sum())
    assert lat.delay_hist(curve[:, :1]).tolist() == [1, 3, 5, 0] and lat.total_delay(curve[:, :1]) == 13
    with pytest.raises(ValueError):   # a receipt before the message exists
        lat.total_delay(curve, np.array([0, 3, 1]))
    with pytest.raises(ValueError):
        lat.delay_hist(curve, inject[:2])
    with pytest.raises(ValueError):
        lat.delay_hist(curve[0], None)
