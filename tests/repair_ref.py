"""Anti-entropy repair as a numpy round loop over a
first-receipt matrix: the reference tests/test_gpu_repair.py compares the
engine with, written from the normative text alone (its own copies of both
draws, no engine code).  It is lossy_ref.run plus `period`, `rseed` and the
repair record; test_repair_ref.py pins it: period 0 is lossy_ref.run, with
every arc open repair changes no first receipt of the C oracle's flood, and on
a path its partners and offers follow from the draw alone.

  round r   up_r, I_r, frontier_r, sends, open_r(u, v): lossy_ref's
            repair round   iff period > 0 and (r + 1) % period == 0; then
            i_r(v)    = below(draw(stream_key(rseed, 0x400 + r), v), deg_in(v)), deg_in(v) > 0
            p_r(v)    = col[row_ptr[v] + i_r(v)]
            x_r(v)    = v up, deg_in(v) > 0, p_r(v) up, open_r(p_r(v), v)
            offer_r[v] = seen_r[p_r(v)] & ~seen_r[v] if x_r(v), else empty
                         (seen_r: first <= r, before any receipt of E_r)
            next[v]   = (OR_{u in In(v), open_r(u, v)} frontier_r[u] | offer_r[v]) & ~seen[v], v up
            first[v][k] = r + 1 for k in next[v]
            exchanges_r = #{v : x_r(v)},  lines_r = sum_v |offer_r[v]|
  the run ends after the first round whose last max(period, 1) rounds all lie
  at or after max(inject) and all have no new bit.
"""
import numpy as np

from lossy_ref import GOLDEN, MASK, NEVER, _mix, _mix_int, arc_open

STREAM_REPAIR = 0x400


def is_repair_round(r, period):
    return period > 0 and (r + 1) % period == 0


def partner_index(rseed, r, v, deg):
    """i_r(v) for arrays of global ids and in-degrees in [1, 2^32) (this file's own copy of the draw)"""
    v, deg = np.broadcast_arrays(np.asarray(v).astype(np.uint64), np.asarray(deg).astype(np.uint64))
    key = _mix_int((rseed & MASK) ^ _mix_int(STREAM_REPAIR + r))
    with np.errstate(over="ignore"):
        d = _mix(np.uint64(key) + v * GOLDEN)
        lo, hi = d & np.uint64(0xFFFFFFFF), d >> np.uint64(32)
        return ((hi * deg + ((lo * deg) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def partner_index_int(rseed, r, v, deg):
    """the same for one vertex, in Python integers"""
    key = _mix_int((rseed & MASK) ^ _mix_int(STREAM_REPAIR + r))
    return (_mix_int((key + v * int(GOLDEN)) & MASK) * deg) >> 64


def partners(g, rseed, r):
    """p_r(v) for every vertex, -1 without an in-neighbour"""
    rp = np.asarray(g.row_ptr, np.int64)
    col = np.asarray(g.col, np.int64)
    deg = np.diff(rp)
    out = np.full(deg.size, -1, np.int64)
    has = np.nonzero(deg > 0)[0]
    if has.size:
        out[has] = col[rp[has] + partner_index(rseed, r, has, deg[has])]
    return out


def run(g, origin, inject=None, p=0.0, seed=0, crash_at=None, max_rounds=254, period=0, rseed=0,
        quiet_reset_at=None):
    """lossy_ref.run's result plus "repair" (uint64 [rounds][2]: exchanges,
    lines) and the two counts in every round's stats.  p = 0.0 is "loss off".
    quiet_reset_at = c: the count of silent rounds starts over before round c
    is counted -- what a checkpoint restored at round c does to the rule."""
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
    quiet = 0
    for r in range(max_rounds):
        up = crash_at > r
        st = dict(round=r, injected=0, lost=0, new_bits=0, receivers=0, sends=0, active=0,
                  crashed=int((crash_at == r).sum()), exchanges=0, lines=0)
        for k in np.nonzero(inj == r)[0]:
            if up[origin[k]]:
                first[origin[k], k] = r
                st["injected"] += 1
            else:
                st["lost"] += 1
        held = first != NEVER                        # seen_r: after L_r and I_r, before E_r's receipts
        F = (first == r) & up[:, None]
        cnt = F.sum(axis=1)
        st["sends"] = int((cnt * deg_out).sum())
        st["active"] = int((cnt > 0).sum())
        senders = np.nonzero(cnt)[0]
        forwards += deg_out[senders] @ F[senders]
        cand = np.zeros((n, m), bool)                # gossip term | offer, before & ~seen
        live = (cnt[src] > 0) & up[dst]
        a = np.nonzero(live)[0]
        if a.size:
            a = a[arc_open(seed, r, src[a], dst[a], p)]
        if a.size:
            bits = np.packbits(F, axis=1)
            d = dst[a]                               # (CSR order: sorted by receiver)
            starts = np.concatenate([[0], np.nonzero(np.diff(d))[0] + 1])
            got = np.bitwise_or.reduceat(bits[src[a]], starts, axis=0)
            cand[d[starts]] = np.unpackbits(got, axis=1)[:, :m].astype(bool)
        if is_repair_round(r, period):
            pr = partners(g, rseed, r)
            v = np.nonzero(up & (pr >= 0))[0]
            v = v[up[pr[v]]]
            v = v[arc_open(seed, r, pr[v], v, p)]
            offer = held[pr[v]] & ~held[v]
            st["exchanges"] = int(v.size)
            st["lines"] = int(offer.sum())
            cand[v] |= offer
        new = cand & ~held & up[:, None]
        first[new] = r + 1
        st["new_bits"] = int(new.sum())
        st["receivers"] = int(new.any(axis=1).sum())
        stats.append(st)
        if r == quiet_reset_at:
            quiet = 0
        quiet = quiet + 1 if st["new_bits"] == 0 and r >= last else 0
        if quiet >= max(period, 1):
            break
    held = first != NEVER
    return {"rounds": len(stats), "stats": stats, "first": first, "seenpop": held.sum(axis=1).astype(np.int64),
            "coverage": held.sum(axis=0).astype(np.uint64), "forwards": forwards.astype(np.uint64),
            "repair": np.array([[s["exchanges"], s["lines"]] for s in stats], np.uint64).reshape(-1, 2)}
