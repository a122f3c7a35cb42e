"""Reading the per-peer fresh deliveries (GossipEngine.fresh_sent() /
fresh_recv(), csrc/fresh.hip) beside the traffic record (load_sent() /
load_recv(), load.py).

fresh_sent[u] is the sends of peer u that delivered a message the receiver did
not hold, fresh_recv[v] the arrivals at v that carried one -- the lines of the
reference's arrival logs (Peer.py:206, Peer.py:286) that were news.  The rest
is redundancy: flooding a power-law overlay sends every message over every
link.  These helpers answer who carries the news and who the duplicates; the
by-degree and concentration views are load.by_degree / load.concentration on
their results.
"""
import numpy as np

from .load import by_degree, concentration  # noqa: F401  (the same views, on these arrays)


def _minus(total, fresh, what):
    total = np.asarray(total).astype(np.int64)
    fresh = np.asarray(fresh).astype(np.int64)
    if total.shape != fresh.shape or total.ndim != 1:
        raise ValueError(f"{what} must be [n]")
    rest = total - fresh
    if (rest < 0).any():
        raise ValueError("more fresh deliveries than lines: arrays of different runs")
    return rest


def wasted(sent, fresh_sent):
    """Peer u's sends that told the receiver nothing new (or reached a crashed
    peer): sent - fresh_sent, int64 [n]."""
    return _minus(sent, fresh_sent, "sent and fresh_sent")


def stale(recv, fresh_recv):
    """Arrivals at peer v of a message it already held: recv - fresh_recv,
    int64 [n]."""
    return _minus(recv, fresh_recv, "recv and fresh_recv")


def efficiency(fresh, total):
    """fresh / total per peer, float64 [n]; 0.0 where total is 0."""
    fresh = np.asarray(fresh).astype(np.float64)
    total = np.asarray(total).astype(np.float64)
    if fresh.shape != total.shape:
        raise ValueError("fresh and total must have one shape")
    if (fresh > total).any():
        raise ValueError("more fresh deliveries than lines: arrays of different runs")
    return np.divide(fresh, total, out=np.zeros(total.shape), where=total > 0)


def relative_redundancy(sent, new_receipts):
    """The run's relative message redundancy: sent.sum() / new_receipts - 1,
    the sends per first receipt beyond the one a spanning tree would need
    (new_receipts: the sum of the rounds' new_bits).  0.0 when nothing was
    received."""
    total = int(np.asarray(sent).astype(np.int64).sum())
    new_receipts = int(new_receipts)
    if new_receipts < 0:
        raise ValueError("new_receipts must be >= 0")
    if new_receipts == 0:
        return 0.0
    return total / new_receipts - 1.0
