"""Expected fresh-delivery curves, from the oracle's outputs
alone -- oracle.run(..., want_first=True): its first-receipt matrix -- and
load_ref.crash_rounds for who was up when; never from the engine.  Shared by
test_fresh_curve_ref.py (CPU: against a per-delivery replay) and
test_gpu_fresh_curve.py.

Arc u -> v (u in In(v)) counts for column k at row first[u][k] + 1 iff

    first[u][k] != 255,  first[v][k] == first[u][k] + 1,  u up in round first[u][k]

An injection at v has no deliverer: no in-neighbour holds k before its inject
round.  Evaluated round by round over bit-packed rows (first == r of the
senders that are up, first == r + 1 of the receivers), by blocks of the arcs
whose two ends both have such a row; only the nonzero words of a block's
row pairs are unpacked into bit columns.
"""
import numpy as np

import load_ref

ARC_BLOCK = 1 << 13


def _packed(first, r):
    """bit-packed rows of first == r as u64 words (message k: word k // 64),
    and the vertices that have one"""
    bits = np.packbits(first == r, axis=1)
    pad = -bits.shape[1] % 8
    if pad:
        bits = np.pad(bits, ((0, 0), (0, pad)))
    bits = np.ascontiguousarray(bits).view(np.uint64)
    return bits, bits.any(axis=1)


def _columns(x, m):
    """per-message counts of the set bits of the u64 rows x [arcs][words]"""
    w, a = np.nonzero(x.T)                                   # (sorted by word)
    per_word = np.zeros((x.shape[1], 64), np.int64)
    if a.size:
        # back to the bytes np.packbits wrote: unpacked bit i of word w is message 64 w + i
        bits = np.unpackbits(np.ascontiguousarray(x[a, w]).view(np.uint8).reshape(-1, 8), axis=1)
        ws, starts = np.unique(w, return_index=True)
        per_word[ws] = np.add.reduceat(bits, starts, axis=0, dtype=np.int64)
    return per_word.reshape(-1)[:m]


def curve(g, ref, crashes=(), churn=False, p_fail=0.0, churn_seed=0, rounds=None, words=None):
    """{"curve": int64 [R + 1][m] after the run's first R = `rounds` rounds (all
    of them by default), "per_round": the arrays after each round ([r + 2][m]
    after round r), "crashed_at", "live_arcs": per round, the arcs whose two
    ends both have a row, "columns": the messages the arrays hold}.  words: the
    64-message words to evaluate (a big shape's sample; the arrays then hold
    those columns only, in order); all of them by default."""
    n = int(g.n)
    rp = np.asarray(g.row_ptr, np.int64)
    src = np.asarray(g.col, np.int64)                       # arc j: src[j] -> dst[j]
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    R = ref["rounds"] if rounds is None else int(rounds)
    if R > ref["rounds"]:
        raise ValueError("more rounds than the oracle ran")
    first = ref["first"]
    m = first.shape[1]
    crashed_at = load_ref.crash_rounds(n, ref["rounds"], crashes, churn, p_fail, churn_seed)
    columns = np.arange(m)
    if words is not None:
        words = np.asarray(sorted(words), np.int64)
        columns = (words[:, None] * 64 + np.arange(64)).reshape(-1)
        if columns.max() >= m:
            raise ValueError("words past the last message")
        m = columns.size
    out = np.zeros((R + 1, m), np.int64)
    per_round, arcs = [], []
    nxt = _packed(first, 0) if R > 0 else None
    for r in range(R):
        fbits, fany = nxt                                    # first == r
        nxt = _packed(first, r + 1)
        nbits, nany = nxt                                    # first == r + 1
        live = np.nonzero((fany & (crashed_at > r))[src] & nany[dst])[0]
        arcs.append(int(live.size))
        for k0 in range(0, live.size, ARC_BLOCK):
            j = live[k0:k0 + ARC_BLOCK]
            if words is None:
                out[r + 1] += _columns(fbits[src[j]] & nbits[dst[j]], m)
            else:
                out[r + 1] += _columns(fbits[src[j]][:, words] & nbits[dst[j]][:, words], m)
        per_round.append(out[:r + 2].copy())
    return {"curve": out, "per_round": per_round, "crashed_at": crashed_at, "live_arcs": arcs, "columns": columns}


def double_star(pkg, leaves):
    """hubs A = 0 and B = 1, each adjacent to all of the leaves 2 .. leaves + 1 (undirected)"""
    n = leaves + 2
    deg = np.array([leaves, leaves] + [2] * leaves, np.int64)
    rp = np.concatenate([[0], deg.cumsum()])
    leaf_ids = np.arange(2, n, dtype=np.int32)
    col = np.concatenate([leaf_ids, leaf_ids, np.tile(np.array([0, 1], np.int32), leaves)])
    return pkg.CSR(n, rp, col, False)


def double_star_expected(leaves, origin_is_leaf):
    """The double star's array by hand, all messages injected in round 0, one
    column per entry of origin_is_leaf.  From a hub: its `leaves` sends of round
    0 are all news, then every leaf tells the other hub at once (`leaves`
    deliverers of one receipt), and that hub's sends of round 2 tell nobody
    anything.  From a leaf: both hubs in round 0, then each hub tells the
    leaves - 1 other leaves, who all hear it twice."""
    hub = [0, leaves, leaves, 0]
    leaf = [0, 2, 2 * (leaves - 1), 0]
    return np.array([leaf if c else hub for c in origin_is_leaf], np.int64).T
