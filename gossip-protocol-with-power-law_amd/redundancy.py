"""Reading the per-peer fresh deliveries (GossipEngine.fresh_sent() /
fresh_recv(), csrc/fresh.hip) beside the traffic record (load_sent() /
load_recv(), load.py).

fresh_sent[u] is the sends of peer u that delivered a message the receiver did
not hold, fresh_recv[v] the arrivals at v that carried one -- the lines of the
reference's arrival logs (Peer.py:206, Peer.py:286) that were news.  The rest
is redundancy: flooding a power-law overlay sends every message over every
link.  These helpers answer who carries the news and who the duplicates; the
by-degree and concentration views are load.by_degree / load.concentration on
their results.  The second half reads the same news per message and round:
GossipEngine.fresh_curve() (csrc/fresh_curve.hip) beside curve(), coverage()
and forwards() -- how many deliverers a first receipt of message k had, and
how many of its sends were wasted.
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


# -- per message: the fresh-delivery curve (GossipEngine.fresh_curve(), -------
# csrc/fresh_curve.hip) beside curve(), coverage() and forwards()

def _curve2d(x, what):
    x = np.asarray(x)
    if x.ndim != 2 or x.shape[0] < 1:
        raise ValueError(f"{what} must be [rounds + 1, m]")
    return x.astype(np.int64)


def _per_message(x, m, what):
    x = np.asarray(x).astype(np.int64)
    if x.shape != (m,):
        raise ValueError(f"{what} must be [m] with m = {m}")
    if (x < 0).any():
        raise ValueError(f"{what} must be >= 0")
    return x


def message_deliverers(fresh_curve):
    """The run's news deliveries of every message: the column sums of
    fresh_curve, int64 [m].  (Their sum is fresh_recv.sum().)"""
    fc = _curve2d(fresh_curve, "fresh_curve")
    if fc[0].any():
        raise ValueError("fresh_curve[0] must be 0: an injection has no deliverer")
    return fc.sum(axis=0)


def deliverers_per_receipt(fresh_curve, coverage):
    """Deliverers per first receipt of every message over the run: the column
    sums of fresh_curve divided by coverage - 1 (the origin's copy has no
    deliverer), float64 [m], >= 1 where defined; 0.0 where coverage - 1 <= 0 (a
    lost message, or one nobody else received)."""
    d = message_deliverers(fresh_curve)
    recv = _per_message(coverage, d.size, "coverage") - 1
    if (d < np.maximum(recv, 0)).any():
        raise ValueError("more receipts than deliveries allow: arrays of different runs")
    if (d[recv <= 0] != 0).any():
        raise ValueError("deliveries of a message nobody received: arrays of different runs")
    return np.divide(d, recv, out=np.zeros(d.shape), where=recv > 0)


def message_redundancy(forwards, coverage):
    """Per-message relative redundancy: forwards[k] / (coverage[k] - 1) - 1, the
    sends of message k per first receipt beyond the one a spanning tree would
    need -- relative_redundancy for one message.  float64 [m]; 0.0 where
    coverage - 1 <= 0."""
    f = np.asarray(forwards)
    if f.ndim != 1:
        raise ValueError("forwards must be [m]")
    f = _per_message(f, f.size, "forwards")
    recv = _per_message(coverage, f.size, "coverage") - 1
    if (f < np.maximum(recv, 0)).any():
        raise ValueError("more receipts than sends allow: arrays of different runs")
    return np.divide(f, recv, out=np.zeros(f.shape, np.float64), where=recv > 0) - (recv > 0)


def deliverers_by_round(fresh_curve, curve):
    """fresh_curve[R] / curve[R] row by row: the deliverers per first receipt of
    message k at receipt round R, float64 [rounds + 1, m], for plotting beside
    spread.py's views; 0.0 where curve[R][k] is 0.  A receipt without a
    deliverer is the origin's own, one per message and row at most."""
    fc = _curve2d(fresh_curve, "fresh_curve")
    cv = _curve2d(curve, "curve")
    if fc.shape != cv.shape:
        raise ValueError("fresh_curve and curve must have one shape")
    if fc[0].any():
        raise ValueError("fresh_curve[0] must be 0: an injection has no deliverer")
    if (fc < 0).any() or (cv < 0).any():
        raise ValueError("counts must be >= 0")
    if (cv - fc > 1).any():
        raise ValueError("more receipts than deliveries allow: arrays of different runs")
    if (fc[cv == 0] != 0).any():
        raise ValueError("deliveries without a receipt: arrays of different runs")
    return np.divide(fc, cv, out=np.zeros(fc.shape, np.float64), where=cv > 0)
