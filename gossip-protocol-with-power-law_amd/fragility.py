"""Reading the delivery multiplicity record (GossipEngine.mult_hist() /
sole_recv() / sole_sent() / sole_bins(), csrc/mult.hip).

A first receipt's multiplicity is the number of in-neighbours that delivered it
in the round it was news: the arrival lines of one message at one peer in that
round (Peer.py:206, Peer.py:286).  A receipt with ten deliverers survives nine
crashed neighbours; a receipt with one hangs on a single link and a single
peer.  These helpers answer the power-law overlay's "robust yet fragile"
question -- hubs deliver most of the news, but are they the only deliverer, or
merely one of many? -- from the histogram and the per-peer sole counts.  Pure
numpy; every function validates its shapes and raises ValueError on arrays that
cannot belong to one run.
"""
import numpy as np

from .latency import degree_bin

MULT_BINS = 17       # gp_read_mult_hist: injections, 1 .. 15 deliverers, 16 or more
BINS, COLS = 32, 4   # gp_read_sole_bins: degree bins x (peers, receipts, sole receipts, sole deliveries)


def _hist(mult_hist):
    h = np.asarray(mult_hist)
    if h.shape != (MULT_BINS,) or h.dtype.kind not in "ui":
        raise ValueError(f"a mult_hist is an integer array [{MULT_BINS}]")
    if h.dtype.kind == "i" and h.size and h.min() < 0:
        raise ValueError("mult_hist is negative somewhere")
    return h.astype(np.uint64)


def _vec(x, name, n=None):
    a = np.asarray(x)
    if a.ndim != 1 or a.dtype.kind not in "ui":
        raise ValueError(f"{name} must be an integer array [vertices]")
    if a.dtype.kind == "i" and a.size and a.min() < 0:
        raise ValueError(f"{name} is negative somewhere")
    a = a.astype(np.int64)
    if n is not None and a.size != n:
        raise ValueError(f"{name} has {a.size} entries, expected {n}: arrays of different runs")
    return a


def sole_share(mult_hist):
    """float: the share of the expansion's first receipts (bins 1 .. 16; the
    injections of bin 0 have no deliverer) that had exactly one deliverer; NaN
    for a run without such receipts."""
    h = _hist(mult_hist)
    tot = int(h[1:].sum())
    return int(h[1]) / tot if tot else float("nan")


def at_least(mult_hist, c):
    """int: the first receipts with c or more deliverers, c in 0 .. 16 (0: every
    receipt, the injections included; 16: the saturated bin)."""
    h = _hist(mult_hist)
    if int(c) != c or not 0 <= int(c) < MULT_BINS:
        raise ValueError(f"c must be an integer in 0 .. {MULT_BINS - 1}: larger counts are one bin")
    return int(h[int(c):].sum())


def combine(hists):
    """uint64 [17]: the histogram of several message shards of one run -- they
    hold disjoint sets of receipts, so the bins add."""
    hs = [_hist(h) for h in hists]
    if not hs:
        raise ValueError("no histogram")
    out = np.zeros(MULT_BINS, np.uint64)
    for h in hs:
        out += h
    return out


def _sum_by(b, x):
    s = np.zeros(BINS, np.int64)   # (integer adds: bincount's weights are float64)
    np.add.at(s, b, x)
    return s


def bins(deg, seenpop, sole_recv, sole_sent):
    """uint64 [32][4], the numpy twin of GossipEngine.sole_bins(): row b holds
    the vertices with latency.degree_bin(deg) = b -- peers, receipts (sum
    seenpop), sum sole_recv, sum sole_sent.  deg is the in-list length."""
    sp = _vec(seenpop, "seenpop")
    sr = _vec(sole_recv, "sole_recv", sp.size)
    ss = _vec(sole_sent, "sole_sent", sp.size)
    if (sr > sp).any():
        raise ValueError("more sole receipts than receipts at a peer: arrays of different runs")
    if int(sr.sum()) != int(ss.sum()):
        raise ValueError("every sole receipt has one sole deliverer: sum sole_recv != sum sole_sent")
    b = degree_bin(_vec(deg, "deg", sp.size))
    out = np.zeros((BINS, COLS), np.uint64)
    out[:, 0] = np.bincount(b, minlength=BINS)
    out[:, 1] = _sum_by(b, sp)
    out[:, 2] = _sum_by(b, sr)
    out[:, 3] = _sum_by(b, ss)
    return out


def _table(table):
    t = np.asarray(table)
    if t.shape != (BINS, COLS) or t.dtype.kind not in "ui":
        raise ValueError(f"a sole_bins table is an integer array [{BINS}][{COLS}]")
    if t.dtype.kind == "i" and t.min() < 0:
        raise ValueError("a sole_bins table is not negative")
    t = t.astype(np.uint64)
    if (t[:, 2] > t[:, 1]).any() or ((t[:, 0] == 0) & t[:, 1:].any(axis=1)).any():
        raise ValueError("not a sole_bins table (sole receipts <= receipts, nothing in a bin without peers)")
    if int(t[:, 2].sum()) != int(t[:, 3].sum()):
        raise ValueError("not a sole_bins table (sum of sole receipts != sum of sole deliveries)")
    return t


def by_degree(table):
    """The populated rows of a sole_bins table, as a list of dicts: bin, the
    bin's degree range [deg_lo, deg_hi], peers, receipts, sole_share (sole
    receipts per receipt: how much of what these peers hold hung on one
    deliverer; NaN without receipts), sole_per_peer (sole deliveries per peer:
    how much news each of them alone carried) and sent_share (the bin's part of
    all sole deliveries; NaN when there are none)."""
    t = _table(table)
    all_sent = int(t[:, 3].sum())
    out = []
    for b in range(BINS):
        peers, receipts, srecv, ssent = (int(x) for x in t[b])
        if peers == 0:
            continue
        out.append(dict(bin=b, deg_lo=0 if b == 0 else 1 << b, deg_hi=1 if b == 0 else (2 << b) - 1, peers=peers,
                        receipts=receipts, sole_share=srecv / receipts if receipts else float("nan"),
                        sole_per_peer=ssent / peers, sent_share=ssent / all_sent if all_sent else float("nan")))
    return out
