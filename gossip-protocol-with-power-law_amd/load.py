"""Reading the per-peer traffic record (GossipEngine.load_sent() /
load_recv() / seenpop(), csrc/load.hip).

sent[u] is the gossip lines peer u put on the wire and recv[v] the lines that
arrived at v, duplicates included -- the totals of what each reference peer
logs line by line (Peer.py:206 and Peer.py:286 log every arriving message with
its sender, Peer.py:402-404 send on every outgoing link).  These helpers turn
them into what one asks of a power-law overlay: how much of the arriving
traffic was redundant, how load grows with degree, and how much of it the hubs
carry.
"""
import numpy as np


def duplicates(recv, seenpop, own):
    """Arrivals that were not first receipts: recv - (seenpop - own), int64 [n].

    seenpop[v] is |Message-List(v)| and own[v] the messages injected at v (they
    entered its list without arriving).  Without liveness own is
    np.bincount(origin, minlength=n).  With liveness a message whose origin was
    down at its inject round never existed (gp_round_stats.lost): the caller
    leaves those messages out of `own`."""
    recv = np.asarray(recv).astype(np.int64)
    first = np.asarray(seenpop).astype(np.int64) - np.asarray(own).astype(np.int64)
    if recv.shape != first.shape or recv.ndim != 1:
        raise ValueError("recv, seenpop and own must be [n]")
    if (first < 0).any():
        raise ValueError("own exceeds seenpop: a lost message was counted as injected")
    dup = recv - first
    if (dup < 0).any():
        raise ValueError("fewer arrivals than first receipts: arrays of different runs")
    return dup


def by_degree(values, deg, bins=32):
    """Per geometric degree class (the binning of degree.ccdf): the class's
    lower bound, its vertex count, and the mean and max of `values` over it.
    Class i holds the vertices with lo[i] <= deg < lo[i + 1] (the last one is
    open); vertices of degree 0 are in no class.  A class without a vertex has
    count 0, mean 0.0 and max 0.  Returns (lo int64, count int64, mean float64,
    max int64), one entry per class."""
    values = np.asarray(values)
    deg = np.asarray(deg, dtype=np.int64)
    if values.shape != deg.shape or deg.ndim != 1:
        raise ValueError("values and deg must be [n]")
    keep = deg > 0
    if not keep.any():
        z = np.zeros(0, np.int64)
        return z, z.copy(), np.zeros(0), z.copy()
    v = values[keep].astype(np.int64)
    d = deg[keep]
    lo = np.unique(np.geomspace(1, d.max(), bins).astype(np.int64))
    cls = np.searchsorted(lo, d, side="right") - 1
    count = np.bincount(cls, minlength=lo.size).astype(np.int64)
    total = np.bincount(cls, weights=v.astype(np.float64), minlength=lo.size)
    mean = np.divide(total, count, out=np.zeros(lo.size), where=count > 0)
    vmax = np.zeros(lo.size, np.int64)
    np.maximum.at(vmax, cls, v)
    return lo, count, mean, vmax


def concentration(values, top=0.01):
    """How unevenly `values` is spread: {"top_share": the share of the total
    carried by the ceil(top * n) largest entries, "max_over_mean": max / mean}.
    Both are 0.0 for an all-zero (or empty) input."""
    v = np.asarray(values).astype(np.float64).ravel()
    if not 0.0 < float(top) <= 1.0:
        raise ValueError("top must be in (0, 1]")
    total = float(v.sum())
    if v.size == 0 or total <= 0.0:
        return {"top_share": 0.0, "max_over_mean": 0.0}
    k = min(v.size, max(1, int(np.ceil(float(top) * v.size - 1e-9))))
    part = np.partition(v, v.size - k)[v.size - k:]
    return {"top_share": float(part.sum()) / total, "max_over_mean": float(v.max()) / (total / v.size)}
