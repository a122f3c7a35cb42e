"""Expected per-peer traffic totals, reconstructed from the
oracle's outputs alone -- oracle.run(..., want_first=True): its first-receipt
matrix, per-round stats and reports -- never from the engine.  Shared by
test_load_ref.py (CPU: against a per-delivery replay) and test_gpu_load.py.

  crash round    from the explicit crashes; with churn, from the oracle
                 harness's own draw for the vertices still up;
  removal round  the round of a vertex's first entry in the oracle's reports;
  per round r    F_r[u]        = (first[u] == r).sum() * up_r[u]
                 deg_live_r[u] = out-degree - out-neighbours removed by round r
                 sent += F_r * deg_live_r
                 recv += up_r * (in-CSR matvec of F_r)

The reconstruction pins itself to the oracle in every round and raises
otherwise: sum F_r * deg_live_r == stats[r].sends, (F_r > 0).sum() ==
stats[r].active.
"""
import math

import numpy as np

NEVER = 1 << 30


def crash_rounds(n, rounds, crashes=(), churn=False, p_fail=0.0, churn_seed=0):
    """Round in which each vertex crashes (NEVER: it stays up)."""
    from oracle import harness
    at = np.full(n, NEVER, np.int64)
    by_round = {}
    for v, r in crashes:
        by_round.setdefault(int(r), []).append(int(v))
    thr = int(math.ldexp(p_fail, 64)) if churn else 0
    for r in range(rounds):
        for v in by_round.get(r, ()):
            if at[v] == NEVER:
                at[v] = r
        if thr:
            for v in np.nonzero(at == NEVER)[0]:
                if harness.draw(churn_seed, 0x100 + r, int(v)) < thr:
                    at[v] = r
    return at


def removal_rounds(n, reports):
    at = np.full(n, NEVER, np.int64)
    for dead, _reporter, r in np.asarray(reports).reshape(-1, 3).tolist():
        at[dead] = min(at[dead], r)
    return at


def row_sums(row_ptr, col, x):
    c = np.concatenate([[0], np.cumsum(x[col], dtype=np.int64)])
    return c[row_ptr[1:]] - c[row_ptr[:-1]]


def frontier_counts(first, rounds):
    """cnt[u][r] = messages u first held in round r (an injection at r
    included), r < rounds: int64 [n][rounds], by blocks of rows."""
    n, m = first.shape
    out = np.zeros((n, rounds), np.int64)
    step = max(1, (1 << 24) // max(m, 1))
    for v0 in range(0, n, step):
        blk = first[v0:v0 + step].astype(np.int32)
        k = blk.shape[0]
        blk += (np.arange(k, dtype=np.int32) * 256)[:, None]
        out[v0:v0 + k] = np.bincount(blk.ravel(), minlength=k * 256).reshape(k, 256)[:, :rounds]
    return out


def totals(g, ref, crashes=(), churn=False, p_fail=0.0, churn_seed=0, rounds=None):
    """{"sent", "recv"}: int64 [n] after the run's first `rounds` rounds (all of
    them by default), "per_round": the pairs after each round, "crashed_at",
    "removed_at"."""
    n = int(g.n)
    rp = np.asarray(g.row_ptr, np.int64)
    col = np.asarray(g.col, np.int64)
    R = ref["rounds"] if rounds is None else int(rounds)
    if R > ref["rounds"]:
        raise ValueError("more rounds than the oracle ran")
    first = ref["first"]
    crashed_at = crash_rounds(n, ref["rounds"], crashes, churn, p_fail, churn_seed)
    removed_at = removal_rounds(n, ref["reports"])
    if ((removed_at != NEVER) & (removed_at <= crashed_at)).any():
        raise AssertionError("a vertex was removed before it crashed")
    deg_live = (np.bincount(col, minlength=n) if g.directed else np.diff(rp)).astype(np.int64)
    sent = np.zeros(n, np.int64)
    recv = np.zeros(n, np.int64)
    per_round = []
    counts = frontier_counts(first, min(R, 255))
    for r in range(R):
        for w in np.nonzero(removed_at == r)[0]:   # the seed drops every link into w
            np.subtract.at(deg_live, col[rp[w]:rp[w + 1]], 1)
        up = crashed_at > r
        F = counts[:, r] * up   # (first == r).sum(axis=1): 255 = never is no round
        st = ref["stats"][r]
        if int((F * deg_live).sum()) != st["sends"]:
            raise AssertionError(f"round {r}: sends {int((F * deg_live).sum())} != oracle {st['sends']}")
        if int((F > 0).sum()) != st["active"]:
            raise AssertionError(f"round {r}: active {int((F > 0).sum())} != oracle {st['active']}")
        if int((~up & (crashed_at == r)).sum()) != st["crashed"]:
            raise AssertionError(f"round {r}: crashed != oracle {st['crashed']}")
        sent += F * deg_live
        recv += up * row_sums(rp, col, F)
        per_round.append((sent.copy(), recv.copy()))
    return {"sent": sent, "recv": recv, "per_round": per_round, "crashed_at": crashed_at,
            "removed_at": removed_at}
