"""Expected per-peer receipt delays, from the oracle's outputs
alone -- oracle.run(..., want_first=True): its first-receipt matrix -- and the
message table; never from the engine.  Shared by test_delay_ref.py (CPU:
against a per-receipt replay) and test_gpu_delay.py.

    delay_sum[v] = sum_{k : first[v][k] != 255} (first[v][k] - inject[k])
    delay_max[v] = max_{k : first[v][k] != 255} (first[v][k] - inject[k]),  0 if v holds nothing

After R rounds the record holds the receipts with first <= R.
"""
import numpy as np

BINS, COLS = 32, 5


def _inject(inject, m):
    return np.zeros(m, np.int64) if inject is None else np.asarray(inject, np.int64)


ROW_BLOCK = 8192   # vertices per step: a wide matrix is walked in blocks of rows


def _upto(first, inj, R):
    parts = [_upto_block(first[v0:v0 + ROW_BLOCK], inj, R) for v0 in range(0, first.shape[0], ROW_BLOCK)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def _upto_block(first, inj, R):
    held = (first != 255) & (first <= min(R, 254))
    held &= ~((first == R) & (inj[None, :] == R))   # round R's injections are not made yet (delay 0: seenpop alone)
    # int16 holds every delay (<= 254); the sums are taken in int64
    d = np.where(held, first.astype(np.int16) - inj.astype(np.int16)[None, :], np.int16(0))
    assert (d >= 0).all(), "a receipt before its message's inject round"
    return d.sum(axis=1, dtype=np.int64), d.max(axis=1, initial=0).astype(np.int64), held.sum(axis=1, dtype=np.int64)


def totals(ref, inject, rounds=None):
    """{"sum", "max": int64 [n] after the run's first `rounds` rounds (all of
    them by default), "seenpop": the number of terms, "per_round": [(sum, max,
    seenpop)] after each round}."""
    first = ref["first"]
    inj = _inject(inject, first.shape[1])
    R = ref["rounds"] if rounds is None else int(rounds)
    if R > ref["rounds"]:
        raise ValueError("more rounds than the oracle ran")
    s, mx, sp = _upto(first, inj, R)
    return {"sum": s, "max": mx, "seenpop": sp, "per_round": _PerRound(first, inj, R)}


class _PerRound:
    """per_round[r] = (sum, max, seenpop) after round r, evaluated when asked
    for (a wide matrix takes a moment per round)"""

    def __init__(self, first, inj, R):
        self.first, self.inj, self.R = first, inj, R

    def __len__(self):
        return self.R

    def __getitem__(self, r):
        if not 0 <= r < self.R:
            raise IndexError(r)
        return _upto(self.first, self.inj, r + 1)


def degree_bin(deg):
    return np.array([0 if d <= 1 else int(d).bit_length() - 1 for d in np.asarray(deg).tolist()], np.int64)


def bins(g, ref, inject, rounds=None, lo=0, hi=None):
    """uint64 [32][5] by degree bin over the vertices [lo, hi): peers, peers
    reached, receipts, sum delay_sum, max delay_max -- per vertex, in Python
    integers."""
    t = totals(ref, inject, rounds)
    deg = np.diff(np.asarray(g.row_ptr, np.int64))
    hi = int(g.n) if hi is None else hi
    out = [[0] * COLS for _ in range(BINS)]
    b = degree_bin(deg)
    for v in range(lo, hi):
        row = out[int(b[v])]
        sp = int(t["seenpop"][v])
        row[0] += 1
        row[1] += 1 if sp > 0 else 0
        row[2] += sp
        row[3] += int(t["sum"][v])
        row[4] = max(row[4], int(t["max"][v]))
    return np.array(out, np.uint64)
