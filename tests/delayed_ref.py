"""The delayed-link semantics of DESIGN.md §2.2 / §2.6 as a numpy round loop over
a first-receipt matrix: the reference tests/test_gpu_link_delay.py compares the
engine with, written from the normative text alone (its own copy of the draws,
no engine code).  test_delayed_ref.py pins it: with dmax = 1 it reproduces the
C oracle's flood and, with loss, lossy_ref.run; with dmax > 1 its first
receipts are the shortest paths under the delays.

  d(u, v)   = 1 + below(draw(stream_key(seed, 0x300), (min(u, v) << 32) | max(u, v)), dmax)
  round r   up_r[v]        = crash_at[v] > r                  (load_ref.crash_rounds)
            I_r            first[o][k] = r for every message k with inject[k] == r
                           whose origin o is up (injected), else the message is lost
            frontier_r[u]  = {k : first[u][k] == r} for u up in round r, else empty;
                           frontier_s is empty for s < 0
            sends          = sum_u deg_out[u] * |frontier_r[u]|     (attempted, in the send round)
            open_s(u, v)   = draw(stream_key(loss_seed, 0x200 + s), (u << 32) | v) >= thresh
            next[v]        = OR_{u in In(v), open_s(u, v), s = r + 1 - d(u, v)} frontier_s[u] & ~seen[v], v up in round r
            first[v][k]    = r + 1 for k in next[v]
  the run ends after the first round r >= max(inject) with no new bit and no
  sender in any round of [r + 2 - dmax, r].

A line sent in round s by a sender that crashes later still arrives; a receiver
down in the arrival round loses it.  deg_out is the static out-degree, as in
lossy_ref: the liveness tests leave `sends` out.
"""
import math

import numpy as np

MASK = (1 << 64) - 1
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
STREAM_LOSS = 0x200
STREAM_LINK_DELAY = 0x300
NEVER = 255
POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.int64)


def _mix(z):
    z = z + GOLDEN
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _mix_int(x):
    z = (x + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _draw(seed, stream, idx):
    key = _mix_int((seed & MASK) ^ _mix_int(stream))
    with np.errstate(over="ignore"):
        return _mix(np.uint64(key) + idx * GOLDEN)


def arc_delay(seed, u, v, dmax):
    """d(u, v) for arrays of global ids (this file's own copy of the draw; the
    multiply-high goes through Python integers)"""
    u, v = np.broadcast_arrays(np.asarray(u).astype(np.uint64), np.asarray(v).astype(np.uint64))
    idx = (np.minimum(u, v) << np.uint64(32)) | np.maximum(u, v)
    r = _draw(seed, STREAM_LINK_DELAY, idx)
    hi, lo = r >> np.uint64(32), r & np.uint64(0xFFFFFFFF)
    n = np.uint64(dmax)
    return (1 + ((hi * n + ((lo * n) >> np.uint64(32))) >> np.uint64(32))).astype(np.int64)


def arc_delays(g, dmax, seed):
    rp = np.asarray(g.row_ptr, np.int64)
    dst = np.repeat(np.arange(int(g.n), dtype=np.int64), np.diff(rp))
    return arc_delay(seed, np.asarray(g.col, np.int64), dst, dmax)


def threshold(p):
    return int(math.ldexp(p, 64)) if 0.0 < p < 1.0 else 0


def arc_open(seed, r, u, v, p):
    u, v = np.broadcast_arrays(np.asarray(u).astype(np.uint64), np.asarray(v).astype(np.uint64))
    if p >= 1.0:
        return np.zeros(u.shape, bool)
    return _draw(seed, STREAM_LOSS + r, (u << np.uint64(32)) | v) >= np.uint64(threshold(p))


def run(g, origin, inject=None, dmax=1, seed=0, p=None, loss_seed=0, crash_at=None, max_rounds=254):
    """{"rounds", "stats" (injected, lost, new_bits, receivers, sends, active,
    crashed per round), "first" u8 [n][m] (255 = never), "seenpop", "coverage",
    "forwards", "by_delay" (first deliveries per delay value, [dmax + 1])}.
    p: loss probability (None: no loss).  crash_at: int array [n], the round
    each vertex crashes in (None: nobody does)."""
    n = int(g.n)
    rp = np.asarray(g.row_ptr, np.int64)
    src = np.asarray(g.col, np.int64)
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    delay = arc_delay(seed, src, dst, dmax)
    origin = np.asarray(origin, np.int64)
    m = origin.size
    inj = np.zeros(m, np.int64) if inject is None else np.asarray(inject, np.int64)
    last = int(inj.max()) if m else 0
    deg_out = (np.bincount(src, minlength=n) if g.directed else np.diff(rp)).astype(np.int64)
    crash_at = np.full(n, 1 << 30, np.int64) if crash_at is None else np.asarray(crash_at, np.int64)
    first = np.full((n, m), NEVER, np.uint8)
    forwards = np.zeros(m, np.int64)
    by_delay = np.zeros(dmax + 1, np.int64)
    nb = (m + 7) // 8
    hist = {}      # send round s -> (packed frontier rows [n][nb], senders bool [n])
    active = {}    # send round s -> senders
    stats = []
    for r in range(max_rounds):
        up = crash_at > r
        st = dict(round=r, injected=0, lost=0, new_bits=0, receivers=0, sends=0, active=0,
                  crashed=int((crash_at == r).sum()))
        for k in np.nonzero(inj == r)[0]:
            if up[origin[k]]:
                first[origin[k], k] = r
                st["injected"] += 1
            else:
                st["lost"] += 1
        F = (first == r) & up[:, None]
        cnt = F.sum(axis=1)
        st["sends"] = int((cnt * deg_out).sum())
        st["active"] = int((cnt > 0).sum())
        senders = np.nonzero(cnt)[0]
        forwards += deg_out[senders] @ F[senders]
        hist[r] = (np.packbits(F, axis=1) if m else np.zeros((n, 0), np.uint8), cnt > 0)
        active[r] = st["active"]
        hist.pop(r - dmax, None)
        # the arcs that deliver this round: arc j carries frontier_{r + 1 - delay[j]}
        got = np.zeros((n, nb), np.uint8)
        arrived = []   # (d, receivers, their OR over the arcs of delay d)
        for d in range(1, dmax + 1):
            s = r + 1 - d
            if s < 0 or not active[s]:
                continue
            bits, sent = hist[s]
            a = np.nonzero((delay == d) & sent[src] & up[dst])[0]
            if p is not None and a.size:
                a = a[arc_open(loss_seed, s, src[a], dst[a], p)]
            if not a.size:
                continue
            recv = dst[a]                               # (CSR order: sorted by receiver)
            starts = np.concatenate([[0], np.nonzero(np.diff(recv))[0] + 1])
            rows = np.bitwise_or.reduceat(bits[src[a]], starts, axis=0)
            got[recv[starts]] |= rows
            arrived.append((d, recv[starts], rows))
        touched = np.nonzero(got.any(axis=1))[0]
        if touched.size:
            sub = first[touched]
            new = np.unpackbits(got[touched], axis=1)[:, :m].astype(bool) & (sub == NEVER)
            sub[new] = r + 1
            first[touched] = sub
            st["new_bits"] = int(new.sum())
            st["receivers"] = int(new.any(axis=1).sum())
            newp = np.packbits(new, axis=1)
            pos = np.full(n, -1, np.int64)
            pos[touched] = np.arange(touched.size)
            for d, recv, rows in arrived:   # (a bit that arrived over two delays at once counts for both)
                by_delay[d] += int(POP[rows & newp[pos[recv]]].sum())
        stats.append(st)
        if st["new_bits"] == 0 and r >= last and not any(active.get(s, 0) for s in range(r + 2 - dmax, r + 1)):
            break
    held = first != NEVER
    return {"rounds": len(stats), "stats": stats, "first": first, "seenpop": held.sum(axis=1).astype(np.int64),
            "coverage": held.sum(axis=0).astype(np.uint64), "forwards": forwards.astype(np.uint64),
            "by_delay": by_delay}


def shortest(g, delay, origin):
    """int64 [n][m]: dist_d(origin[k], v) under the per-arc delays (numpy
    Bellman-Ford over the in-CSR; a large value where v is unreachable)"""
    n = int(g.n)
    rp = np.asarray(g.row_ptr, np.int64)
    src = np.asarray(g.col, np.int64)
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    origin = np.asarray(origin, np.int64)
    uniq, inv = np.unique(origin, return_inverse=True)
    INF = np.int64(1) << 40
    dist = np.full((n, uniq.size), INF, np.int64)
    dist[uniq, np.arange(uniq.size)] = 0
    delay = np.asarray(delay, np.int64)
    nonempty = np.nonzero(np.diff(rp))[0]
    starts = rp[nonempty]
    while True:
        cand = np.minimum.reduceat(dist[src] + delay[:, None], starts, axis=0)
        new = dist.copy()
        new[nonempty] = np.minimum(new[nonempty], cand)
        if np.array_equal(new, dist):
            break
        dist = new
    return dist[:, inv]
