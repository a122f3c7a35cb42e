"""Expected per-link fresh deliveries, from the oracle's
outputs alone -- oracle.run(..., want_first=True): its first-receipt matrix --
and load_ref.crash_rounds for who was up when; never from the engine.  Shared
by test_link_ref.py (CPU: against a per-delivery replay) and
test_gpu_link_fresh.py.

Arc j of the in-CSR (u = col[j] -> v = the row of j) counts the messages m with

    first[u][m] != 255,  first[v][m] == first[u][m] + 1,  u up in round first[u][m]

and the term belongs to round first[u][m].  An injection at v has no deliverer:
no in-neighbour holds m before its inject round.  Evaluated round by round over
bit-packed rows (first == r of the senders that are up, first == r + 1 of the
receivers), by blocks of the arcs whose two ends both have such a row, so that
per_round[r] is the record after round r.
"""
import numpy as np

import load_ref
from fresh_ref import ARC_BLOCK, _packed, _popcount_rows


def record(g, ref, crashes=(), churn=False, p_fail=0.0, churn_seed=0, rounds=None):
    """{"link": int64 [nnz] link_fresh after the run's first `rounds` rounds
    (all of them by default), "per_round": the array after each round,
    "src", "dst": the arcs' ends, "crashed_at"}."""
    n = int(g.n)
    rp = np.asarray(g.row_ptr, np.int64)
    src = np.asarray(g.col, np.int64)                       # arc j: src[j] -> dst[j]
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    R = ref["rounds"] if rounds is None else int(rounds)
    if R > ref["rounds"]:
        raise ValueError("more rounds than the oracle ran")
    first = ref["first"]
    crashed_at = load_ref.crash_rounds(n, ref["rounds"], crashes, churn, p_fail, churn_seed)
    link = np.zeros(src.size, np.int64)
    per_round = []
    nxt = _packed(first, 0) if R > 0 else None
    for r in range(R):
        fbits, fany = nxt                                    # first == r
        nxt = _packed(first, r + 1)
        nbits, nany = nxt                                    # first == r + 1
        live = np.nonzero((fany & (crashed_at > r))[src] & nany[dst])[0]
        for k0 in range(0, live.size, ARC_BLOCK):
            j = live[k0:k0 + ARC_BLOCK]
            link[j] += _popcount_rows(fbits[src[j]] & nbits[dst[j]])   # (j: distinct arcs)
        per_round.append(link.copy())
    return {"link": link, "per_round": per_round, "src": src, "dst": dst, "crashed_at": crashed_at}


def path(pkg, n):
    """the undirected path 0 - 1 - ... - n - 1"""
    rp = np.array([0] + [1 if v in (0, n - 1) else 2 for v in range(n)], np.int64).cumsum()
    col = np.array([u for v in range(n) for u in (v - 1, v + 1) if 0 <= u < n], np.int32)
    return pkg.CSR(n, rp, col, False)
