"""Expected per-peer delay distributions, from the oracle's
outputs alone -- oracle.run(..., want_first=True): its first-receipt matrix --
and the message table; never from the engine.  Shared by
test_delay_dist_ref.py (CPU: against a per-receipt replay) and
test_gpu_delay_dist.py.

    delay_dist[v][d] = #{ k : first[v][k] != 255, min(first[v][k] - inject[k], 15) = d }

After R rounds the record holds the receipts with first <= R, and round R's
injections are not made yet (the rule of delay_ref.py).
"""
import numpy as np

D = 16
BINS = 32
ROW_BLOCK = 8192   # vertices per step: a wide matrix is walked in blocks of rows


def _inject(inject, m):
    return np.zeros(m, np.int64) if inject is None else np.asarray(inject, np.int64)


def _upto_block(first, inj, R):
    held = (first != 255) & (first <= min(R, 254))
    held &= ~((first == R) & (inj[None, :] == R))   # round R's injections are not made yet
    d = first.astype(np.int16) - inj.astype(np.int16)[None, :]
    assert (d[held] >= 0).all(), "a receipt before its message's inject round"
    # one count per (vertex, column); column D collects what is not held
    cell = np.where(held, np.minimum(d, D - 1), D).astype(np.int32)
    cell += (np.arange(first.shape[0], dtype=np.int32) * (D + 1))[:, None]
    out = np.bincount(cell.ravel(), minlength=first.shape[0] * (D + 1)).reshape(first.shape[0], D + 1)[:, :D]
    return out.astype(np.int64), held.sum(axis=1, dtype=np.int64)


def _upto(first, inj, R):
    parts = [_upto_block(first[v0:v0 + ROW_BLOCK], inj, R) for v0 in range(0, first.shape[0], ROW_BLOCK)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def totals(ref, inject, rounds=None):
    """{"dist": int64 [n][16] after the run's first `rounds` rounds (all of them
    by default), "seenpop": int64 [n], the row sums, "per_round": [(dist,
    seenpop)] after each round}."""
    first = ref["first"]
    inj = _inject(inject, first.shape[1])
    R = ref["rounds"] if rounds is None else int(rounds)
    if R > ref["rounds"]:
        raise ValueError("more rounds than the oracle ran")
    dist, sp = _upto(first, inj, R)
    return {"dist": dist, "seenpop": sp, "per_round": _PerRound(first, inj, R)}


class _PerRound:
    """per_round[r] = (dist, seenpop) after round r, evaluated when asked for"""

    def __init__(self, first, inj, R):
        self.first, self.inj, self.R = first, inj, R

    def __len__(self):
        return self.R

    def __getitem__(self, r):
        if not 0 <= r < self.R:
            raise IndexError(r)
        return _upto(self.first, self.inj, r + 1)


def degree_bin(deg):
    return [0 if d <= 1 else int(d).bit_length() - 1 for d in np.asarray(deg).tolist()]


def bins(g, dist, lo=0, hi=None):
    """uint64 [32][16] by degree bin over the vertices [lo, hi) of `dist`
    ([n][16], as totals gives it) -- per vertex, in Python integers."""
    deg = np.diff(np.asarray(g.row_ptr, np.int64))
    hi = int(g.n) if hi is None else hi
    out = [[0] * D for _ in range(BINS)]
    b = degree_bin(deg)
    rows = np.asarray(dist).tolist()
    for v in range(lo, hi):
        row = out[b[v]]
        for d, x in enumerate(rows[v]):
            row[d] += int(x)
    return np.array(out, np.uint64)
