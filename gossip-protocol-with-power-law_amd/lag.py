"""Delayed links (GossipEngine.link_delay(), csrc/delayed.hip, csrc/link_delay.h).

With delay on, the link between peers u and v takes

    d(u, v) = 1 + below(draw(stream_key(seed, 0x300), (min(u, v) << 32) | max(u, v)), dmax)

rounds, 1 <= dmax <= 8: the line u sends in round s has
receipt round s + d(u, v).  The delay belongs to the unordered pair and the
run.  This module restates the draw in numpy -- arc_delays lists a graph's
delays in the in-CSR's arc order, as GossipEngine.arc_delays() reads them --
and sweeps a run over dmax: how many rounds the news takes, how late it
arrives on average, while coverage stays the flood's.
"""
import numpy as np

STREAM_LINK_DELAY = 0x300   # csrc/link_delay.h
DMAX = 8
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M32 = np.uint64(0xFFFFFFFF)


def _splitmix64(x):
    """splitmix64's output function on a uint64 array (wrapping arithmetic)"""
    z = x + _GOLDEN
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _u64(x, name):
    a = np.asarray(x)
    if a.dtype.kind not in "ui":
        raise ValueError(f"{name} must be integers")
    if a.dtype.kind == "i" and a.size and a.min() < 0:
        raise ValueError(f"{name} is negative somewhere")
    a = a.astype(np.uint64)
    if a.size and a.max() >> np.uint64(32):
        raise ValueError("vertex ids are below 2^32")
    return a


def _check_dmax(dmax):
    dmax = int(dmax)
    if not 1 <= dmax <= DMAX:
        raise ValueError(f"dmax must lie in [1, {DMAX}]")
    return dmax


def key(seed):
    """stream_key(seed, STREAM_LINK_DELAY) as a Python int"""
    with np.errstate(over="ignore"):
        s = _splitmix64(np.array([STREAM_LINK_DELAY], np.uint64))
        return int(_splitmix64(np.array([int(seed) & ((1 << 64) - 1)], np.uint64) ^ s)[0])


def _below(r, n):
    """floor(r * n / 2^64) for a uint64 array r and 1 <= n <= 2^32, exactly"""
    n = np.uint64(n)
    lo = (r & _M32) * n
    return ((r >> np.uint64(32)) * n + (lo >> np.uint64(32))) >> np.uint64(32)


def arc_delay(seed, u, v, dmax):
    """uint8 array: the rounds the link between u[i] and v[i] takes (global
    vertex ids below 2^32; the arrays broadcast against each other)."""
    dmax = _check_dmax(dmax)
    u, v = np.broadcast_arrays(_u64(u, "u"), _u64(v, "v"))
    with np.errstate(over="ignore"):
        idx = (np.minimum(u, v) << np.uint64(32)) | np.maximum(u, v)
        d = _splitmix64(np.uint64(key(seed)) + idx * _GOLDEN)
    return (_below(d, dmax) + np.uint64(1)).astype(np.uint8)


def arc_delays(g, dmax, seed=0):
    """uint8 [nnz]: the delay of every arc of g's in-CSR, in row_ptr / col
    order (sender col[j], receiver the row of j)."""
    rp = np.asarray(g.row_ptr, np.int64)
    recv = np.repeat(np.arange(int(g.n), dtype=np.int64), np.diff(rp))
    return arc_delay(seed, np.asarray(g.col, np.int64), recv, dmax)


def sweep(engine, dmaxes, seed=0, max_rounds=254):
    """For every dmax of `dmaxes`, set link_delay(dmax, seed), reset and run
    the engine's message table once, with track_delay on for the run.  Returns
    a list of dicts {"dmax", "rounds", "coverage" (uint64 [m], peers reached
    per message), "mean_delay" (receipt round - inject round, averaged over
    the first receipts that are no injections; 0.0 without any)}.  The engine
    keeps the last setting and track_delay; link_delay(None) and a reset give
    the flood back."""
    out = []
    engine.track_delay()
    for dmax in dmaxes:
        engine.link_delay(dmax, seed)
        engine.reset()
        stats = engine.run(max_rounds)
        engine.finalize()
        receipts = sum(s["new_bits"] for s in stats)
        total = int(engine.delay_sum().astype(np.uint64).sum())   # (injections have delay 0)
        out.append({"dmax": int(dmax), "rounds": len(stats), "coverage": engine.coverage(),
                    "mean_delay": total / receipts if receipts else 0.0})
    return out
