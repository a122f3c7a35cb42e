"""Reading a spread curve (GossipEngine.curve(), csrc/curve.hip).

curve[r][k] is the number of vertices whose first receipt of message k has
receipt round r -- the aggregate of the per-arrival log each reference peer
keeps (Peer.py:175-216).  These helpers turn it into the two things one plots:
the coverage of each message after each round, and the rounds a message took
to reach a share of the peers, counted from its own inject round.

Column k is message k of the table the engine ran.  If that table was ordered
with GossipEngine.spread_order's permutation p (origin[p], inject_round[p]),
column k is message p[k] of the original table, exactly as for coverage();
pass inject_round[p] here, or undo it with out[p] = result.
"""
import numpy as np


def cumulative(curve):
    """cum[r][k] = vertices holding message k once receipt round r is done
    (int64 [rows][m]); cum[-1] is the coverage after the rounds that ran."""
    c = np.asarray(curve)
    if c.ndim != 2:
        raise ValueError("curve must be [rows][m]")
    return np.cumsum(c.astype(np.int64), axis=0)


def rounds_to_reach(curve, inject_round, frac, of="final"):
    """Per message, the first receipt round, counted from the message's inject
    round, at which its coverage reaches `frac` of its final coverage
    (of="final") or of n vertices (of=n); -1 if it never does -- a lost
    message (an all-zero column) never does.  int64 [m]."""
    cum = cumulative(curve)
    rows, m = cum.shape
    inj = np.asarray(inject_round, dtype=np.int64) if inject_round is not None else np.zeros(m, np.int64)
    if inj.shape != (m,):
        raise ValueError("inject_round must have one entry per curve column")
    if not 0.0 < float(frac) <= 1.0:
        raise ValueError("frac must be in (0, 1]")
    final = cum[-1] if rows else np.zeros(m, np.int64)
    if isinstance(of, str):
        if of != "final":
            raise ValueError('of must be "final" or the vertex count n')
        base = final.astype(np.float64)
    else:
        if int(of) < 1:
            raise ValueError("n must be >= 1")
        base = np.full(m, float(int(of)))
    # integer threshold: the smallest count that is >= frac * base
    need = np.ceil(float(frac) * base - 1e-9).astype(np.int64)
    need = np.maximum(need, 1)
    hit = cum >= need[None, :]
    reached = hit.any(axis=0) & (final > 0)
    first = np.argmax(hit, axis=0).astype(np.int64)
    return np.where(reached, first - inj, -1)
