"""Expected delivery multiplicity, from the oracle's outputs
alone -- oracle.run(..., want_first=True): its first-receipt matrix -- and
load_ref.crash_rounds for who was up when; never from the engine.  Shared by
test_mult_ref.py (CPU: against a per-delivery replay) and test_gpu_mult.py.

For first[v][k] != 255 the deliverers of the receipt (v, k) are the arcs u -> v
(u in In(v), parallel arcs separately) with

    first[u][k] != 255,  first[v][k] == first[u][k] + 1,  u up in round first[u][k]

-- the rules of fresh_ref.py -- and c is their number; c == 0 iff the receipt
is the injection.  Evaluated round by round over bit-packed rows (first == r of
the senders that are up, first == r + 1 of the receivers), by blocks of the
arcs whose two ends both have such a row.  The count per (receiver, message) is
kept bit-sliced too, but not the way the engine keeps it: five plain binary
planes (exact to 31) and an overflow plane, filled four arcs per receiver at a
time (arcs t .. t + 3 of every receiver of a block that has them, together).
"""
import numpy as np

import load_ref
from fresh_ref import _packed, _popcount_rows

ARC_BLOCK = 1 << 16
BINS = 17          # hist[0]: injections; hist[c], c = 1 .. 15; hist[16]: 16 or more
_PLANES = 5        # exact counts 0 .. 31, then sticky


def _popcount(x):
    return int(_popcount_rows(x.reshape(1, -1))[0]) if x.size else 0


class _Counts:
    """per (group, bit) number of rows of a group that have the bit, groups
    given as a sorted id per row: planes[b][group] and an overflow plane"""

    def __init__(self, rows, gid, ngroups):
        W = rows.shape[1]
        self.p = [np.zeros((ngroups, W), np.uint64) for _ in range(_PLANES)]
        self.over = np.zeros((ngroups, W), np.uint64)
        if rows.shape[0] == 0:
            return
        sizes = np.bincount(gid, minlength=ngroups)
        first_of = np.cumsum(sizes) - sizes                # (gid is sorted: a group's rows are consecutive)
        last = rows.shape[0] - 1
        for t in range(0, int(sizes.max()), 4):            # four rows of every group that has them, as one carry-save add
            act = np.nonzero(sizes > t)[0]
            whole = act.size == ngroups
            a = []
            for q in range(4):
                x = np.take(rows, np.minimum(first_of[act] + (t + q), last), axis=0)
                x[sizes[act] <= t + q] = 0
                a.append(x)
            p = self.p if whole else [pl[act] for pl in self.p]
            t1 = a[0] ^ a[1]
            s1 = t1 ^ a[2]
            k1 = (a[0] & a[1]) | (t1 & a[2])               # a0 + a1 + a2 = s1 + 2 k1
            t2 = s1 ^ a[3]
            p0 = t2 ^ p[0]
            k2 = (s1 & a[3]) | (t2 & p[0])                 # s1 + a3 + p0 = p0' + 2 k2
            t3 = k1 ^ k2
            p1 = t3 ^ p[1]
            carry = (k1 & k2) | (t3 & p[1])                # k1 + k2 + p1 = p1' + 2 carry
            out = [p0, p1]
            for b in range(2, _PLANES):
                out.append(p[b] ^ carry)
                carry = p[b] & carry
            if whole:
                self.p = out
                self.over |= carry
            else:
                for b in range(_PLANES):
                    self.p[b][act] = out[b]
                self.over[act] |= carry

    def masks(self):
        """[17] masks: count == c for c = 0 .. 15, then count >= 16"""
        p, free = self.p, ~(self.over | self.p[4])
        lo = [~p[0] & ~p[1], p[0] & ~p[1], ~p[0] & p[1], p[0] & p[1]]
        hi = [free & ~p[2] & ~p[3], free & p[2] & ~p[3], free & ~p[2] & p[3], free & p[2] & p[3]]
        return [lo[c & 3] & hi[c >> 2] for c in range(16)] + [~free]


def totals(g, ref, crashes=(), churn=False, p_fail=0.0, churn_seed=0, rounds=None, chunk=None):
    """{"hist": int64 [17], "sole_recv", "sole_sent": int64 [n]} after the run's
    first `rounds` rounds (all of them by default), "per_round": the triples
    after each round, "crashed_at".  With chunk = C also, over the receivers
    whose in-list is longer than C: "big_hist" (bins 1 .. 16 of their
    receipts) and "cross", the number of their receipts with 2 .. 15
    deliverers that lie in different C-arc chunks of the in-list."""
    n = int(g.n)
    rp = np.asarray(g.row_ptr, np.int64)
    src = np.asarray(g.col, np.int64)                       # arc j: src[j] -> dst[j]
    deg = np.diff(rp)
    dst = np.repeat(np.arange(n, dtype=np.int64), deg)
    pos = np.arange(src.size, dtype=np.int64) - rp[dst]     # place of the arc in its receiver's in-list
    R = ref["rounds"] if rounds is None else int(rounds)
    if R > ref["rounds"]:
        raise ValueError("more rounds than the oracle ran")
    first = ref["first"]
    crashed_at = load_ref.crash_rounds(n, ref["rounds"], crashes, churn, p_fail, churn_seed)
    hist = np.zeros(BINS, np.int64)
    big_hist = np.zeros(BINS, np.int64)
    cross = 0
    sole_recv = np.zeros(n, np.int64)
    sole_sent = np.zeros(n, np.int64)
    per_round = []
    nxt = _packed(first, 0) if R > 0 else None
    for r in range(R):
        fbits, fany = nxt                                    # first == r
        if r == 0:
            pending = _popcount(fbits)                       # nobody delivers in round -1: all injections
        hist[0] += pending                                   # I_r: the receipts of round r nobody delivered
        nxt = _packed(first, r + 1)
        nbits, nany = nxt                                    # first == r + 1
        live = np.nonzero((fany & (crashed_at > r))[src] & nany[dst])[0]   # (in-CSR order: sorted by receiver)
        delivered = 0
        # blocks of whole receivers
        k0 = 0
        while k0 < live.size:
            k1 = min(k0 + ARC_BLOCK, live.size)
            if k1 < live.size:
                vend = dst[live[k1 - 1]]
                k1 = k0 + int(np.searchsorted(dst[live[k0:]], vend, side="right"))
            j = live[k0:k1]
            k0 = k1
            u, v = src[j], dst[j]
            x = fbits[u] & nbits[v]
            vs, gid = np.unique(v, return_inverse=True)
            mk = _Counts(x, gid, vs.size).masks()
            got = [0] + [_popcount(mk[c]) for c in range(1, BINS)]
            hist += got
            delivered += sum(got)
            sole = mk[1]
            sole_recv[vs] += _popcount_rows(sole)
            w = _popcount_rows(fbits[u] & sole[gid])
            sole_sent += np.bincount(u, weights=w, minlength=n).astype(np.int64)
            if chunk is not None:
                bigv = deg[vs] > chunk
                if bigv.any():
                    big_hist += [0] + [_popcount(mk[c][bigv]) for c in range(1, BINS)]
                    # per (receiver, chunk) the OR of the deliveries, then how many chunks hold each bit
                    ck = gid * (int(deg.max()) // chunk + 1) + pos[j] // chunk
                    cstart = np.nonzero(np.r_[True, ck[1:] != ck[:-1]])[0]
                    ors = np.bitwise_or.reduceat(x, cstart, axis=0)
                    ck = _Counts(ors, gid[cstart], vs.size).masks()
                    several = ~(mk[0] | mk[1] | mk[16]) & ~(ck[0] | ck[1])   # 2 .. 15 deliverers, 2 or more chunks
                    cross += _popcount(several[bigv])
        pending = _popcount(nbits) - delivered               # ... of round r + 1: injected then, counted when it runs
        if pending and r + 1 >= ref["rounds"]:
            raise AssertionError("an injection after the oracle's last round")
        per_round.append((hist.copy(), sole_recv.copy(), sole_sent.copy()))
    out = {"hist": hist, "sole_recv": sole_recv, "sole_sent": sole_sent, "per_round": per_round,
           "crashed_at": crashed_at}
    if chunk is not None:
        out["big_hist"] = big_hist
        out["cross"] = cross
    return out


def table(g, seenpop, exp):
    """the sole_bins table of an expected record, the slow way: a loop over the vertices"""
    out = np.zeros((32, 4), np.uint64)
    deg = np.diff(np.asarray(g.row_ptr, np.int64))
    for v in range(int(g.n)):
        b = 0 if deg[v] <= 1 else int(deg[v]).bit_length() - 1
        out[b] += np.array([1, int(seenpop[v]), int(exp["sole_recv"][v]), int(exp["sole_sent"][v])], np.uint64)
    return out
