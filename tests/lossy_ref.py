"""The lossy-link semantics of DESIGN.md §2.2 / §2.6 as a numpy round loop over
a first-receipt matrix: the reference tests/test_gpu_link_loss.py compares the
engine with, written from the normative text alone (its own copy of the draw,
no engine code).  test_lossy_ref.py pins it: with every arc open it reproduces
the C oracle's flood, and on a path its reaches follow from the draw alone.

  round r   up_r[v]        = crash_at[v] > r                  (load_ref.crash_rounds)
            I_r            first[o][k] = r for every message k with inject[k] == r
                           whose origin o is up (injected), else the message is lost
            frontier_r[u]  = {k : first[u][k] == r} for up u, else empty
            sends          = sum_u deg_out[u] * |frontier_r[u]|     (attempted sends)
            open_r(u, v)   = draw(stream_key(seed, 0x200 + r), (u << 32) | v) >= thresh
            next[v]        = OR_{u in In(v), open_r(u, v)} frontier_r[u] & ~seen[v], v up
            first[v][k]    = r + 1 for k in next[v]
  the run ends after the first round r >= max(inject) with no new bit.

deg_out is the static out-degree: under liveness the engine's `sends` follows
the seed's removals (deg_live), which this loop does not model -- the tests
leave `sends` out there.
"""
import math

import numpy as np

MASK = (1 << 64) - 1
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
STREAM_LOSS = 0x200
NEVER = 255


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


def threshold(p):
    return int(math.ldexp(p, 64)) if 0.0 < p < 1.0 else 0


def arc_open(seed, r, u, v, p):
    """open_r(u, v) for arrays of global ids (this file's own copy of the draw)"""
    u, v = np.broadcast_arrays(np.asarray(u).astype(np.uint64), np.asarray(v).astype(np.uint64))
    if p >= 1.0:
        return np.zeros(u.shape, bool)
    key = _mix_int((seed & MASK) ^ _mix_int(STREAM_LOSS + r))
    with np.errstate(over="ignore"):
        d = _mix(np.uint64(key) + ((u << np.uint64(32)) | v) * GOLDEN)
    return d >= np.uint64(threshold(p))


def run(g, origin, inject=None, p=0.0, seed=0, crash_at=None, max_rounds=254):
    """{"rounds", "stats" (injected, lost, new_bits, receivers, sends, active,
    crashed per round), "first" u8 [n][m] (255 = never), "seenpop", "coverage",
    "forwards"}.  crash_at: int array [n], the round each vertex crashes in
    (load_ref.crash_rounds; None: nobody does)."""
    n = int(g.n)
    rp = np.asarray(g.row_ptr, np.int64)
    src = np.asarray(g.col, np.int64)
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    origin = np.asarray(origin, np.int64)
    m = origin.size
    inj = np.zeros(m, np.int64) if inject is None else np.asarray(inject, np.int64)
    last = int(inj.max()) if m else 0
    deg_out = (np.bincount(src, minlength=n) if g.directed else np.diff(rp)).astype(np.int64)
    crash_at = np.full(n, 1 << 30, np.int64) if crash_at is None else np.asarray(crash_at, np.int64)
    first = np.full((n, m), NEVER, np.uint8)
    forwards = np.zeros(m, np.int64)
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
        live = (cnt[src] > 0) & up[dst]
        if live.any():
            a = np.nonzero(live)[0]
            a = a[arc_open(seed, r, src[a], dst[a], p)]
        else:
            a = np.zeros(0, np.int64)
        if a.size:
            bits = np.packbits(F, axis=1)            # [n][ceil(m / 8)]
            d = dst[a]                               # (CSR order: sorted by receiver)
            starts = np.concatenate([[0], np.nonzero(np.diff(d))[0] + 1])
            got = np.bitwise_or.reduceat(bits[src[a]], starts, axis=0)
            recv = d[starts]
            new = np.unpackbits(got, axis=1)[:, :m].astype(bool) & (first[recv] == NEVER)
            sub = first[recv]
            sub[new] = r + 1
            first[recv] = sub
            st["new_bits"] = int(new.sum())
            st["receivers"] = int(new.any(axis=1).sum())
        stats.append(st)
        if st["new_bits"] == 0 and r >= last:
            break
    held = first != NEVER
    return {"rounds": len(stats), "stats": stats, "first": first, "seenpop": held.sum(axis=1).astype(np.int64),
            "coverage": held.sum(axis=0).astype(np.uint64), "forwards": forwards.astype(np.uint64)}
