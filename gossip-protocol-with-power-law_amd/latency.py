"""Reading the per-peer receipt delays (GossipEngine.delay_sum() / delay_max()
/ delay_bins(), csrc/delay.hip).

A receipt delay is first[v][k] - inject_round[k]: how many rounds after message
k was generated peer v heard it -- the time column of the reference's arrival
log (Peer.py:206, Peer.py:286) grouped by the receiving peer.  In the
round-synchronous model it is v's hop distance from the origin on the live
overlay, so with many random origins delay_sum / seenpop is a sampled closeness
and delay_max a sampled eccentricity.  These helpers answer the power-law
question -- do hubs hear early and leaves late? -- and tie the record to the
spread curve.  Pure numpy; every function validates its shapes and raises
ValueError on arrays that cannot belong to one run.

The dist_* helpers read the per-peer delay distributions
(GossipEngine.delay_dist() / delay_dist_bins(), csrc/delay_dist.hip): the same
receipts per delay value, which give each peer's and each degree bin's median
and tail.
"""
from fractions import Fraction

import numpy as np

BINS, COLS = 32, 5   # gp_read_delay_bins: degree bins x (peers, reached, receipts, delay sum, delay max)
MAX_DELAY = 254      # inject rounds are <= 253, receipt rounds <= 254


def _vec(x, name, n=None):
    a = np.asarray(x)
    if a.ndim != 1 or a.dtype.kind not in "ui":
        raise ValueError(f"{name} must be an integer array [vertices]")
    a = a.astype(np.int64)
    if n is not None and a.size != n:
        raise ValueError(f"{name} has {a.size} entries, expected {n}: arrays of different runs")
    if a.size and a.min() < 0:
        raise ValueError(f"{name} is negative somewhere")
    return a


def _record(seenpop, delay_sum, delay_max=None):
    sp = _vec(seenpop, "seenpop")
    ds = _vec(delay_sum, "delay_sum", sp.size)
    if (ds[sp == 0] != 0).any():
        raise ValueError("a peer that holds nothing has a delay: arrays of different runs")
    if (ds > sp * MAX_DELAY).any():
        raise ValueError(f"a mean delay above {MAX_DELAY}: not a delay_sum array")
    if delay_max is None:
        return sp, ds, None
    dm = _vec(delay_max, "delay_max", sp.size)
    if dm.size and dm.max() > MAX_DELAY:
        raise ValueError(f"a delay above {MAX_DELAY}: not a delay_max array")
    if (dm * sp < ds).any() or (dm > ds).any():
        raise ValueError("delay_max is not the maximum of delay_sum's terms: arrays of different runs")
    return sp, ds, dm


def mean_delay(delay_sum, seenpop):
    """float64 [vertices]: delay_sum / seenpop, NaN for a peer that holds
    nothing (never reached)."""
    sp, ds, _ = _record(seenpop, delay_sum)
    out = np.full(sp.size, np.nan)
    np.divide(ds, sp, out=out, where=sp > 0)
    return out


def degree_bin(deg):
    """int64: 0 for deg <= 1, else floor(log2(deg)) -- the row of a vertex in
    delay_bins()."""
    d = _vec(np.atleast_1d(deg), "deg")
    if d.size and d.max() >= 1 << BINS:
        raise ValueError("a degree of 2^32 or more: not an overlay's")
    out = np.zeros(d.size, np.int64)
    for k in range(1, BINS):   # integer shifts: np.log2 of a float is not exact near powers of two
        out += (d >> k) > 0
    return out


def bins(deg, seenpop, delay_sum, delay_max):
    """uint64 [32][5], the numpy twin of GossipEngine.delay_bins(): row b holds
    the vertices with degree_bin(deg) = b -- peers, peers reached (seenpop >
    0), receipts (sum seenpop), sum delay_sum, max delay_max."""
    sp, ds, dm = _record(seenpop, delay_sum, delay_max)
    b = degree_bin(_vec(deg, "deg", sp.size))
    out = np.zeros((BINS, COLS), np.uint64)
    out[:, 0] = np.bincount(b, minlength=BINS)
    out[:, 1] = np.bincount(b[sp > 0], minlength=BINS)
    out[:, 2] = _sum_by(b, sp)
    out[:, 3] = _sum_by(b, ds)
    mx = np.zeros(BINS, np.int64)
    np.maximum.at(mx, b, dm)
    out[:, 4] = mx
    return out


def _sum_by(b, x):
    s = np.zeros(BINS, np.int64)   # (integer adds: bincount's weights are float64)
    np.add.at(s, b, x)
    return s


def combine(tables, disjoint=True):
    """The table of several contexts: columns 0-3 add over partition ranks
    (disjoint=True: disjoint vertex sets); over message shards of one vertex
    set (disjoint=False) the peers are the first table's, receipts and delay
    sums add, and `reached` is not a function of the shards' tables (set to
    0).  Column 4 takes the maximum."""
    ts = [_table(t) for t in tables]
    if not ts:
        raise ValueError("no table")
    out = np.zeros((BINS, COLS), np.uint64)
    for t in ts:
        out[:, :4] += t[:, :4]
        out[:, 4] = np.maximum(out[:, 4], t[:, 4])
    if not disjoint:
        if any((t[:, 0] != ts[0][:, 0]).any() for t in ts):
            raise ValueError("shards of one vertex set have the same peers per bin")
        out[:, 0] = ts[0][:, 0]
        out[:, 1] = 0
    return out


def _table(table):
    t = np.asarray(table)
    if t.shape != (BINS, COLS) or t.dtype.kind not in "ui":
        raise ValueError(f"a delay_bins table is an integer array [{BINS}][{COLS}]")
    t = t.astype(np.uint64)
    if (t[:, 1] > t[:, 0]).any() or (t[:, 2] < t[:, 1]).any() or (t[:, 4] > MAX_DELAY).any():
        raise ValueError("not a delay_bins table (reached <= peers, receipts >= reached, max <= 254)")
    return t


def by_degree(table):
    """The populated rows of a delay_bins table, as a list of dicts: bin, the
    bin's degree range [deg_lo, deg_hi], peers, reach (share of the bin's peers
    that hold anything), mean_delay (sum of delays / receipts, NaN without
    receipts) and max_delay."""
    t = _table(table)
    out = []
    for b in range(BINS):
        peers, reached, receipts, dsum, dmax = (int(x) for x in t[b])
        if peers == 0:
            continue
        out.append(dict(bin=b, deg_lo=0 if b == 0 else 1 << b, deg_hi=1 if b == 0 else (2 << b) - 1, peers=peers,
                        reach=reached / peers, mean_delay=dsum / receipts if receipts else float("nan"),
                        max_delay=dmax))
    return out


def _curve(curve, inject_round):
    c = np.asarray(curve)
    if c.ndim != 2 or c.dtype.kind not in "ui":
        raise ValueError("curve must be an integer array [rounds + 1][m]")
    m = c.shape[1]
    inj = np.zeros(m, np.int64) if inject_round is None else _vec(inject_round, "inject_round", m)
    c = c.astype(np.int64)
    rounds = np.arange(c.shape[0], dtype=np.int64)[:, None]
    if (c[rounds < inj[None, :]] != 0).any():
        raise ValueError("a receipt before its message's inject round: curve and inject_round of different runs")
    return c, rounds - inj[None, :]


def delay_hist(curve, inject_round=None):
    """uint64 [rounds + 1]: the run's receipts per delay -- hist[d] = receipts
    with receipt round - inject round = d, injections (d = 0) included."""
    c, d = _curve(curve, inject_round)
    ok = d >= 0
    h = np.zeros(c.shape[0], np.int64)   # (integer adds: bincount's weights are float64)
    np.add.at(h, d[ok], c[ok])
    return h.astype(np.uint64)


def total_delay(curve, inject_round=None):
    """int: sum_R sum_k (R - inject_round[k]) * curve[R][k] -- over a
    single-rank run exactly sum(delay_sum())."""
    c, d = _curve(curve, inject_round)
    return int((np.where(d >= 0, d, 0) * c).sum())


# -- delay distributions (delay_dist(), delay_dist_bins()) ------------------------

DIST_BINS = 16       # columns of a delay_dist row: delays 0 .. 14, 15 or more
DIST_LAST = DIST_BINS - 1


def _dist(dist, name="dist", rows=None):
    a = np.asarray(dist)
    if a.ndim != 2 or a.shape[1] != DIST_BINS or a.dtype.kind not in "ui":
        raise ValueError(f"{name} must be an integer array [rows][{DIST_BINS}]")
    a = a.astype(np.int64)
    if rows is not None and a.shape[0] != rows:
        raise ValueError(f"{name} has {a.shape[0]} rows, expected {rows}: arrays of different runs")
    if a.size and a.min() < 0:
        raise ValueError(f"{name} is negative somewhere")
    return a


def dist_quantile(dist, q, flag=False):
    """float64 [rows]: the q-quantile of every row's delays by the lower-value
    rule -- the smallest d with cumsum(row)[d] >= ceil(q * total), at least the
    first receipt.  NaN for a row without receipts (a peer never reached).  A
    quantile that falls in the last column is only known to be >= 15 and is
    returned as 15; flag=True returns (values, saturated) with a bool array
    that marks those rows.  Works on delay_dist() and on a delay_dist_bins()
    table alike."""
    a = _dist(dist)
    if not 0 <= q <= 1:
        raise ValueError("q must be in [0, 1]")
    f = Fraction(q).limit_denominator(10 ** 9)   # (0.9 * 10 is not 9 in floating point)
    total = a.sum(axis=1)
    rank = np.maximum((f.numerator * total + f.denominator - 1) // f.denominator, 1)
    idx = (np.cumsum(a, axis=1) < rank[:, None]).sum(axis=1)   # first column whose cumsum reaches the rank
    out = np.full(a.shape[0], np.nan)
    ok = total > 0
    out[ok] = idx[ok]
    return (out, ok & (idx == DIST_LAST)) if flag else out


def dist_bins(deg, dist):
    """uint64 [32][16], the numpy twin of GossipEngine.delay_dist_bins(): row b
    sums the rows of the vertices with degree_bin(deg) = b."""
    a = _dist(dist)
    b = degree_bin(_vec(deg, "deg", a.shape[0]))
    out = np.zeros((BINS, DIST_BINS), np.int64)
    for k in np.unique(b):   # (integer adds, a bin at a time: np.add.at is slow on millions of rows)
        out[k] = a[b == k].sum(axis=0)
    return out.astype(np.uint64)


def _dist_table(table):
    t = np.asarray(table)
    if t.shape != (BINS, DIST_BINS) or t.dtype.kind not in "ui":
        raise ValueError(f"a delay_dist_bins table is an integer array [{BINS}][{DIST_BINS}]")
    if t.size and t.min() < 0:
        raise ValueError("a delay_dist_bins table is negative somewhere")
    return t.astype(np.int64)


def dist_by_degree(table, qs=(0.5, 0.9, 0.99)):
    """The rows of a delay_dist_bins table that hold receipts, as a list of
    dicts: bin, the bin's degree range [deg_lo, deg_hi] (as by_degree),
    receipts, mean_delay (the last column taken as 15: a lower bound when
    `saturated`), one key per quantile -- "p50", "p90", "p99" for the default
    qs -- and saturated: whether any of them fell in the last column."""
    t = _dist_table(table)
    cols = [dist_quantile(t, q, flag=True) for q in qs]
    out = []
    for b in range(BINS):
        receipts = int(t[b].sum())
        if receipts == 0:
            continue
        row = dict(bin=b, deg_lo=0 if b == 0 else 1 << b, deg_hi=1 if b == 0 else (2 << b) - 1, receipts=receipts,
                   mean_delay=int((t[b] * np.arange(DIST_BINS)).sum()) / receipts)
        for q, (val, _) in zip(qs, cols):
            row[f"p{100 * q:g}"] = int(val[b])
        row["saturated"] = any(bool(sat[b]) for _, sat in cols)
        out.append(row)
    return out


def dist_combine(arrays):
    """int64: the element-wise sum of several contexts' delay_dist() arrays (or
    delay_dist_bins() tables) -- message shards of one vertex set.  Added in
    int64: nothing promises that the shards' u16 cells add up within u16."""
    arrs = [np.asarray(a) for a in arrays]
    if not arrs:
        raise ValueError("no array")
    for a in arrs:
        if a.ndim != 2 or a.shape != arrs[0].shape or a.shape[1] != DIST_BINS or a.dtype.kind not in "ui":
            raise ValueError(f"shards' arrays are integer arrays of one shape [rows][{DIST_BINS}]")
    out = np.zeros(arrs[0].shape, np.int64)
    for a in arrs:
        out += a.astype(np.int64)
    return out


def dist_check(dist, seenpop, delay_sum=None, delay_max=None):
    """Raise ValueError unless the arrays can belong to one run: every row of
    dist sums to seenpop; with delay_sum, a row with an empty last column has
    sum d * dist[d] = delay_sum and any other at most delay_sum; with
    delay_max, the largest occupied column is delay_max, or delay_max >= 15
    where the last column is occupied."""
    sp = _vec(seenpop, "seenpop")
    a = _dist(dist, rows=sp.size)
    if (a.sum(axis=1) != sp).any():
        raise ValueError("a row of dist does not sum to seenpop: arrays of different runs")
    open_ = a[:, DIST_LAST] == 0
    if delay_sum is not None:
        ds = _vec(delay_sum, "delay_sum", sp.size)
        weighted = (a * np.arange(DIST_BINS)).sum(axis=1)
        if (weighted[open_] != ds[open_]).any():
            raise ValueError("sum d * dist[d] is not delay_sum where no delay reached 15: arrays of different runs")
        if (weighted[~open_] > ds[~open_]).any():
            raise ValueError("sum d * dist[d] exceeds delay_sum: arrays of different runs")
    if delay_max is not None:
        dm = _vec(delay_max, "delay_max", sp.size)
        top = np.where(a > 0, np.arange(DIST_BINS)[None, :], 0).max(axis=1, initial=0)
        if (top[open_] != dm[open_]).any():
            raise ValueError("the largest occupied column is not delay_max: arrays of different runs")
        if (dm[~open_] < DIST_LAST).any():
            raise ValueError("receipts of 15 rounds or later with a delay_max below 15: arrays of different runs")
