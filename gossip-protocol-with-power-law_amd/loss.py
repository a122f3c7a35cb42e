"""Lossy links (GossipEngine.link_loss(), csrc/lossy.hip, csrc/link_loss.h).

With loss on, the line peer u puts on link u -> v in round r arrives iff

    draw(stream_key(seed, 0x200 + r), (u << 32) | v) >= threshold(p)

(DESIGN.md §2.2, §2.6).  A peer still sends a message only in the one round
after it first received it, so a dropped line is lost for good (the reference's
send loop, Peer.py:402-404, sends once per link).  This module restates the
draw in numpy -- arc_open lists the links that were open in a round -- and
sweeps a run over loss probabilities: the survival curve of the flood's
redundancy.

Coverage is not monotone in p for a fixed seed: receiving earlier moves a
peer's one forwarding round onto another set of open arcs.
"""
import math

import numpy as np

STREAM_LOSS = 0x200   # + round (csrc/link_loss.h)
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


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
    return a.astype(np.uint64)


def threshold(p):
    """The 64-bit threshold of 0 < p < 1 (an arc is open iff its draw is >=
    it), int(ldexp(p, 64)); 0 for p = 0 -- every arc open -- and for p = 1,
    where every arc is closed and nothing is drawn."""
    p = float(p)
    if not 0.0 <= p <= 1.0:   # (NaN fails both comparisons)
        raise ValueError("p must lie in [0, 1]")
    return int(math.ldexp(p, 64)) if 0.0 < p < 1.0 else 0


def round_key(seed, r):
    """stream_key(seed, STREAM_LOSS + r) as a Python int"""
    with np.errstate(over="ignore"):
        s = _splitmix64(np.array([STREAM_LOSS + int(r)], np.uint64))
        return int(_splitmix64(np.array([int(seed) & ((1 << 64) - 1)], np.uint64) ^ s)[0])


def arc_open(seed, r, senders, receivers, p):
    """bool array: link senders[i] -> receivers[i] delivers in round r (global
    vertex ids below 2^32; the arrays broadcast against each other)."""
    u, v = _u64(senders, "senders"), _u64(receivers, "receivers")
    if (u.size and u.max() >> np.uint64(32)) or (v.size and v.max() >> np.uint64(32)):
        raise ValueError("vertex ids are below 2^32")
    thr = threshold(p)
    u, v = np.broadcast_arrays(u, v)
    if float(p) >= 1.0:
        return np.zeros(u.shape, bool)
    with np.errstate(over="ignore"):
        idx = (u << np.uint64(32)) | v
        d = _splitmix64(np.uint64(round_key(seed, r)) + idx * _GOLDEN)
    return d >= np.uint64(thr)


def sweep(engine, ps, seed=0, max_rounds=254):
    """The survival curve: for every p of `ps`, set link_loss(p, seed), reset
    and run the engine's message table once.  Returns a list of dicts
    {"p", "rounds", "coverage" (uint64 [m], peers reached per message),
    "reached" (share of the (peer, message) cells reached)}.  The engine keeps
    the last setting; link_loss(None) and a reset give the flood back."""
    out = []
    for p in ps:
        engine.link_loss(p, seed)
        engine.reset()
        stats = engine.run(max_rounds)
        engine.finalize()
        cov = engine.coverage()
        cells = float(engine.n) * float(engine.m)
        out.append({"p": float(p), "rounds": len(stats), "coverage": cov,
                    "reached": float(cov.sum()) / cells if cells else 0.0})
    return out
