"""Anti-entropy repair (GossipEngine.repair(), csrc/repair.hip, csrc/repair_draw.h).

Over lossy links a dropped line is lost for good (loss.py).  With repair on,
round r is a repair round iff (r + 1) % period == 0, and in one every up peer v
with an in-neighbour pulls the whole Message-List of

    p_r(v) = col[row_ptr[v] + below(draw(stream_key(seed, 0x400 + r), v), deg_in(v))]

over the link p_r(v) -> v, if the partner is up and the round's loss draw
leaves that link open.  What the exchange brings is a
first receipt like any other: v forwards it once, so repair restarts the flood.
This module restates the partner draw in numpy and sweeps a run over repair
periods: what repair buys back, and what it costs in exchanges and in lines.

A run stops after `period` silent rounds.  With one random partner that is the
stopping rule, not convergence: another draw could still repair something.
"""
import numpy as np

STREAM_REPAIR = 0x400   # + round (csrc/repair_draw.h)
PERIOD_MAX = 64
_MASK = (1 << 64) - 1
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def _splitmix64(x):
    """splitmix64's output function on a uint64 array (wrapping arithmetic)"""
    z = x + _GOLDEN
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def is_repair_round(r, period):
    """round r of a run with this period reconciles (period 0 or None: never)"""
    return bool(period) and (int(r) + 1) % int(period) == 0


def round_key(seed, r):
    """stream_key(seed, STREAM_REPAIR + r) as a Python int"""
    with np.errstate(over="ignore"):
        s = _splitmix64(np.array([STREAM_REPAIR + int(r)], np.uint64))
        return int(_splitmix64(np.array([int(seed) & _MASK], np.uint64) ^ s)[0])


def _below(d, n):
    """floor(d * n / 2^64) for uint64 arrays d and n < 2^32, without 128-bit products"""
    lo, hi = d & np.uint64(0xFFFFFFFF), d >> np.uint64(32)
    return (hi * n + ((lo * n) >> np.uint64(32))) >> np.uint64(32)


def partner_index(seed, r, v, deg):
    """Index into v's in-list of its partner in round r (global vertex ids v,
    in-degrees 0 < deg < 2^32; the arrays broadcast against each other)."""
    v, deg = np.broadcast_arrays(np.asarray(v), np.asarray(deg))
    if v.size and (v.min() < 0 or deg.min() <= 0 or int(deg.max()) >> 32):
        raise ValueError("vertex ids are non-negative and in-degrees lie in [1, 2^32)")
    with np.errstate(over="ignore"):
        d = _splitmix64(np.uint64(round_key(seed, r)) + v.astype(np.uint64) * _GOLDEN)
        return _below(d, deg.astype(np.uint64)).astype(np.int64)


def partners(csr, seed, r):
    """int64 [n]: p_r(v) for every vertex of the in-CSR `csr` (row_ptr, col as
    loaded or built: GossipEngine.graph()), -1 where v has no in-neighbour."""
    rp = np.asarray(csr.row_ptr, np.int64)
    col = np.asarray(csr.col, np.int64)
    deg = np.diff(rp)
    out = np.full(deg.size, -1, np.int64)
    has = np.nonzero(deg > 0)[0]
    if has.size:
        out[has] = col[rp[has] + partner_index(seed, r, has, deg[has])]
    return out


def sweep(engine, periods, seed=0, max_rounds=254):
    """What repair buys and costs: for every period of `periods` (None or 0:
    no repair), set repair(period, seed), reset and run the engine's message
    table once, on top of whatever link_loss is set.  Returns a list of dicts
    {"period", "rounds", "coverage" (uint64 [m]), "reached" (share of the
    (peer, message) cells reached), "exchanges", "lines" (totals over the
    run)}.  A run that reaches max_rounds (254 at most) is cut there.  The
    engine keeps the last setting; repair(None) and a reset give the run
    without repair back."""
    out = []
    for period in periods:
        engine.repair(period or None, seed)
        engine.reset()
        stats = engine.run(max_rounds)
        engine.finalize()
        cov = engine.coverage()
        rec = engine.repair_record() if period else np.zeros((0, 2), np.uint64)
        cells = float(engine.n) * float(engine.m)
        out.append({"period": int(period or 0), "rounds": len(stats), "coverage": cov,
                    "reached": float(cov.sum()) / cells if cells else 0.0,
                    "exchanges": int(rec[:, 0].sum()), "lines": int(rec[:, 1].sum())})
    return out
