"""redundancy.py's helpers on hand-made arrays (CPU)."""
import numpy as np
import pytest


def test_wasted_and_stale(pkg):
    red = pkg.redundancy
    sent = np.array([10, 0, 7, 3], np.uint64)
    fresh = np.array([4, 0, 7, 0], np.uint64)
    w = red.wasted(sent, fresh)
    assert w.dtype == np.int64 and w.tolist() == [6, 0, 0, 3]
    s = red.stale(sent, fresh)
    assert s.dtype == np.int64 and s.tolist() == [6, 0, 0, 3]
    assert red.wasted(np.zeros(3, np.uint64), np.zeros(3, np.uint64)).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        red.wasted(sent, np.array([11, 0, 0, 0], np.uint64))   # more fresh than sent
    with pytest.raises(ValueError):
        red.stale(sent[:3], fresh)
    with pytest.raises(ValueError):
        red.stale(sent.reshape(2, 2), fresh.reshape(2, 2))


def test_efficiency(pkg):
    red = pkg.redundancy
    e = red.efficiency(np.array([4, 0, 7, 0], np.uint64), np.array([10, 0, 7, 3], np.uint64))
    assert e.dtype == np.float64 and e.tolist() == [0.4, 0.0, 1.0, 0.0]      # 0 where total is 0
    assert red.efficiency(np.zeros(0), np.zeros(0)).size == 0
    assert not red.efficiency(np.zeros(5, np.uint64), np.zeros(5, np.uint64)).any()
    with pytest.raises(ValueError):
        red.efficiency(np.array([1, 2]), np.array([1]))
    with pytest.raises(ValueError):
        red.efficiency(np.array([2]), np.array([1]))


def test_relative_redundancy(pkg):
    red = pkg.redundancy
    assert red.relative_redundancy(np.array([6, 2, 2], np.uint64), 4) == 1.5
    assert red.relative_redundancy(np.array([3, 1], np.uint64), 4) == 0.0     # a tree: one send per receipt
    assert red.relative_redundancy(np.zeros(4, np.uint64), 0) == 0.0
    assert red.relative_redundancy(np.array([5], np.uint64), 0) == 0.0        # sends to crashed peers only
    with pytest.raises(ValueError):
        red.relative_redundancy(np.array([1]), -1)


def test_by_degree_views_are_loads(pkg):
    """the by-degree and concentration views are load.py's, on these arrays"""
    red = pkg.redundancy
    assert red.by_degree is pkg.load.by_degree and red.concentration is pkg.load.concentration
    deg = np.array([1, 2, 3, 0, 64, 64, 1, 5])
    sent = np.array([10, 20, 60, 0, 1000, 3000, 30, 8], np.uint64)
    fresh = np.array([10, 10, 30, 0, 100, 300, 30, 2], np.uint64)
    lo, count, mean, vmax = red.by_degree(red.wasted(sent, fresh), deg, bins=4)
    assert lo.tolist() == [1, 4, 16, 64] and count.tolist() == [4, 1, 0, 2]
    assert mean.tolist() == [10.0, 6.0, 0.0, 1800.0] and vmax.tolist() == [30, 6, 0, 2700]
    c = red.concentration(red.wasted(sent, fresh), top=0.125)
    assert c["top_share"] == 2700 / 3646
