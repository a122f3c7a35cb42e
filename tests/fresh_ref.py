"""Expected per-peer fresh deliveries, from the oracle's
outputs alone -- oracle.run(..., want_first=True): its first-receipt matrix --
and load_ref.crash_rounds for who was up when; never from the engine.  Shared
by test_fresh_ref.py (CPU: against a per-delivery replay) and
test_gpu_fresh.py.

Arc u -> v (u in In(v)) contributes the messages m with

    first[u][m] != 255,  first[v][m] == first[u][m] + 1,  u up in round first[u][m]

to fresh_sent[u] and to fresh_recv[v], and the term belongs to round
first[u][m].  An injection at v has no deliverer: no in-neighbour holds m
before its inject round.  Evaluated round by round over bit-packed rows
(first == r of the senders that are up, first == r + 1 of the receivers), by
blocks of the arcs whose two ends both have such a row.
"""
import numpy as np

import load_ref

ARC_BLOCK = 1 << 16

if hasattr(np, "bitwise_count"):
    def _popcount_rows(x):
        return np.bitwise_count(x).sum(axis=1, dtype=np.int64)
else:
    _POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)

    def _popcount_rows(x):
        return _POP8[np.ascontiguousarray(x).view(np.uint8)].sum(axis=1, dtype=np.int64)


def _packed(first, r):
    """bit-packed rows of first == r, and the vertices that have one"""
    bits = np.packbits(first == r, axis=1)
    pad = -bits.shape[1] % 8
    if pad:
        bits = np.pad(bits, ((0, 0), (0, pad)))
    bits = np.ascontiguousarray(bits).view(np.uint64)   # (8 bytes per popcount)
    return bits, bits.any(axis=1)


def totals(g, ref, crashes=(), churn=False, p_fail=0.0, churn_seed=0, rounds=None):
    """{"sent", "recv"}: int64 [n] fresh_sent / fresh_recv after the run's first
    `rounds` rounds (all of them by default), "per_round": the pairs after
    each round, "crashed_at"."""
    n = int(g.n)
    rp = np.asarray(g.row_ptr, np.int64)
    src = np.asarray(g.col, np.int64)                       # arc j: src[j] -> dst[j]
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    R = ref["rounds"] if rounds is None else int(rounds)
    if R > ref["rounds"]:
        raise ValueError("more rounds than the oracle ran")
    first = ref["first"]
    crashed_at = load_ref.crash_rounds(n, ref["rounds"], crashes, churn, p_fail, churn_seed)
    sent = np.zeros(n, np.int64)
    recv = np.zeros(n, np.int64)
    per_round = []
    nxt = _packed(first, 0) if R > 0 else None
    for r in range(R):
        fbits, fany = nxt                                    # first == r
        nxt = _packed(first, r + 1)
        nbits, nany = nxt                                    # first == r + 1
        live = np.nonzero((fany & (crashed_at > r))[src] & nany[dst])[0]
        for k0 in range(0, live.size, ARC_BLOCK):
            j = live[k0:k0 + ARC_BLOCK]
            u, v = src[j], dst[j]
            c = _popcount_rows(fbits[u] & nbits[v])
            sent += np.bincount(u, weights=c, minlength=n).astype(np.int64)
            recv += np.bincount(v, weights=c, minlength=n).astype(np.int64)
        per_round.append((sent.copy(), recv.copy()))
    return {"sent": sent, "recv": recv, "per_round": per_round, "crashed_at": crashed_at}
