"""fragility.py, the helpers that read the delivery multiplicity record, on
hand-made arrays (CPU): the share of receipts with one deliverer, the tail of
the histogram, the numpy twin of the device's degree table with degree 0, the
by-degree reading, and the shards' combine."""
import math

import numpy as np
import pytest

# injections, then receipts with 1 .. 15 deliverers, then 16 or more
HIST = np.array([5, 40, 20, 10] + [1] * 12 + [8], np.uint64)

# five peers: a leaf, a hub, an isolated vertex (degree 0, unreached), an origin
# that holds only its own message, a degree-1 peer never reached
DEG = np.array([2, 9, 0, 3, 1])
SEENPOP = np.array([3, 6, 0, 1, 0], np.uint32)
SRECV = np.array([3, 1, 0, 0, 0], np.uint32)
SSENT = np.array([0, 3, 0, 1, 0], np.uint64)


def test_sole_share(pkg):
    fr = pkg.fragility
    assert fr.sole_share(HIST) == 40 / 90                      # the injections are no expansion receipts
    assert fr.sole_share(HIST.astype(np.int64)) == 40 / 90
    assert math.isnan(fr.sole_share(np.array([7] + [0] * 16)))  # nothing but injections
    assert fr.sole_share([0, 3] + [0] * 15) == 1.0
    for bad in (HIST[:16], np.zeros((17, 1), np.uint64), HIST.astype(np.float64), -HIST.astype(np.int64)):
        with pytest.raises(ValueError):
            fr.sole_share(bad)


def test_at_least(pkg):
    fr = pkg.fragility
    assert fr.at_least(HIST, 0) == int(HIST.sum()) == 95
    assert fr.at_least(HIST, 1) == 90 and fr.at_least(HIST, 2) == 50 and fr.at_least(HIST, 3) == 30
    assert fr.at_least(HIST, 16) == 8
    for c in range(16):
        assert fr.at_least(HIST, c) - fr.at_least(HIST, c + 1) == int(HIST[c])
    for bad in (17, -1, 1.5):
        with pytest.raises(ValueError):
            fr.at_least(HIST, bad)


def test_combine(pkg):
    fr = pkg.fragility
    a = np.arange(17, dtype=np.uint64)
    out = fr.combine([HIST, a, a])
    assert out.dtype == np.uint64 and np.array_equal(out, HIST + 2 * a)
    assert np.array_equal(fr.combine([HIST]), HIST)
    assert np.array_equal(fr.combine(iter([HIST.tolist(), a])), HIST + a)
    with pytest.raises(ValueError):
        fr.combine([])
    with pytest.raises(ValueError):
        fr.combine([HIST, a[:16]])


def test_bins(pkg):
    fr = pkg.fragility
    t = fr.bins(DEG, SEENPOP, SRECV, SSENT)
    assert t.dtype == np.uint64 and t.shape == (32, 4) == (fr.BINS, fr.COLS)
    # bin 0: degrees 0 and 1; bin 1: degrees 2 and 3; bin 3: degree 9
    assert t[0].tolist() == [2, 0, 0, 0]
    assert t[1].tolist() == [2, 4, 3, 1]
    assert t[3].tolist() == [1, 6, 1, 3]
    assert not t[[2] + list(range(4, 32))].any()
    assert int(t[:, 2].sum()) == int(t[:, 3].sum()) == 4
    # large counts stay exact (integer sums, no float)
    big = fr.bins([4, 5, 1 << 20], [4096, 4096, 0], [4096, 0, 0], [1, 4095, 0])
    assert big[2].tolist() == [2, 8192, 4096, 4096] and big[20].tolist() == [1, 0, 0, 0]
    with pytest.raises(ValueError):
        fr.bins(DEG[:4], SEENPOP, SRECV, SSENT)                 # arrays of different runs
    with pytest.raises(ValueError):
        fr.bins(DEG, SEENPOP, SRECV[:4], SSENT[:4])
    with pytest.raises(ValueError):
        fr.bins(DEG, SEENPOP, np.array([4, 0, 0, 0, 0]), SSENT)   # more sole receipts than receipts
    with pytest.raises(ValueError):
        fr.bins(DEG, SEENPOP, SRECV, np.array([0, 3, 0, 2, 0]))   # the two sides do not add up
    with pytest.raises(ValueError):
        fr.bins(DEG, SEENPOP, SRECV.astype(np.float64), SSENT)


def test_by_degree(pkg):
    fr = pkg.fragility
    rows = fr.by_degree(fr.bins(DEG, SEENPOP, SRECV, SSENT))
    assert [r["bin"] for r in rows] == [0, 1, 3]
    assert [(r["deg_lo"], r["deg_hi"]) for r in rows] == [(0, 1), (2, 3), (8, 15)]
    assert [r["peers"] for r in rows] == [2, 2, 1] and [r["receipts"] for r in rows] == [0, 4, 6]
    assert math.isnan(rows[0]["sole_share"]) and rows[0]["sole_per_peer"] == 0.0
    assert rows[1]["sole_share"] == 3 / 4 and rows[1]["sole_per_peer"] == 0.5 and rows[1]["sent_share"] == 1 / 4
    assert rows[2]["sole_share"] == 1 / 6 and rows[2]["sole_per_peer"] == 3.0 and rows[2]["sent_share"] == 3 / 4
    empty = fr.by_degree(fr.bins(DEG, np.zeros(5, np.uint32), np.zeros(5, np.uint32), np.zeros(5, np.uint64)))
    assert all(math.isnan(r["sole_share"]) and math.isnan(r["sent_share"]) for r in empty)
    bad = fr.bins(DEG, SEENPOP, SRECV, SSENT)
    for cell, value in (((1, 2), 5), ((2, 1), 1), ((3, 3), 9)):   # sole > receipts; a bin without peers; sums differ
        t = bad.copy()
        t[cell] = value
        with pytest.raises(ValueError):
            fr.by_degree(t)
    with pytest.raises(ValueError):
        fr.by_degree(bad[:, :3])
