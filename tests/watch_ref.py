"""Expected watched-peers record, from the oracle's outputs
alone -- oracle.run(..., want_first=True): its first-receipt matrix -- and
load_ref.crash_rounds for who was up when; never from the engine.  Shared by
test_watch_ref.py (CPU: against a per-delivery replay) and test_gpu_watch.py.

With the watch list v_0 .. v_{K-1} and watched arc a = ptr[s] + i the i-th arc
of row v_s of the in-CSR, sender u = col[row_ptr[v_s] + i]:

    watch_first[s][k]   = first[v_s][k]
    watch_arrival[a][k] = first[u][k] + 1   iff first[u][k] != 255 and both u and
                                            v_s are up in round first[u][k]
                        = 255               otherwise

which is load_ref's recv term per (arc, message).
"""
import numpy as np

import load_ref

NEVER = 255


def arcs(g, verts):
    rp = np.asarray(g.row_ptr, np.int64)
    col = np.asarray(g.col, np.int64)
    verts = [int(v) for v in verts]
    ptr = np.zeros(len(verts) + 1, np.int64)
    for s, v in enumerate(verts):
        ptr[s + 1] = ptr[s] + rp[v + 1] - rp[v]
    sender = np.array([int(col[j]) for v in verts for j in range(int(rp[v]), int(rp[v + 1]))], np.int64)
    slot = np.array([s for s, v in enumerate(verts) for _ in range(int(rp[v]), int(rp[v + 1]))], np.int64)
    return ptr, sender, slot


def record(g, ref, verts, crashes=(), churn=False, p_fail=0.0, churn_seed=0):
    """{"ptr": i64 [K + 1], "sender", "slot": i64 [A], "first": u8 [K][m],
    "arrival": u8 [A][m], "crashed_at"} of the whole run."""
    n = int(g.n)
    first = ref["first"]
    verts = np.asarray([int(v) for v in verts], np.int64)
    ptr, sender, slot = arcs(g, verts)
    crashed_at = load_ref.crash_rounds(n, ref["rounds"], crashes, churn, p_fail, churn_seed)
    fu = first[sender].astype(np.int64)                                   # [A][m]
    ok = (fu != NEVER) & (crashed_at[sender][:, None] > fu) & (crashed_at[verts[slot]][:, None] > fu)
    arrival = np.where(ok, fu + 1, NEVER).astype(np.uint8)
    return {"ptr": ptr, "sender": sender, "slot": slot, "first": first[verts].copy(), "arrival": arrival,
            "crashed_at": crashed_at, "verts": verts}


def after(rec, rounds, origin, inject):
    """(first, arrival) as the record stands after `rounds` rounds: the cells
    with value <= rounds, but for the injections of round `rounds` itself"""
    first = rec["first"].copy()
    arrival = rec["arrival"].copy()
    first[first > rounds] = NEVER
    arrival[arrival > rounds] = NEVER
    inj = np.zeros(first.shape[1], np.int64) if inject is None else np.asarray(inject, np.int64)
    origin = np.asarray(origin, np.int64)
    at_origin = rec["verts"][:, None] == origin[None, :]                   # [K][m]
    first[at_origin & (inj[None, :] == rounds) & (first == rounds)] = NEVER
    return first, arrival


def summaries(rec):
    """per slot, from the record alone: lines, fresh, per-arc fresh, sole
    receipts, held -- what load_recv, fresh_recv, link_fresh, sole_recv and
    seenpop hold for the peer"""
    out = []
    for s in range(rec["ptr"].size - 1):
        a = rec["arrival"][rec["ptr"][s]:rec["ptr"][s + 1]]
        f = rec["first"][s]
        got = a != NEVER
        fresh = got & (a == f[None, :])
        held = f != NEVER
        out.append({"lines": int(got.sum()), "fresh": int(fresh.sum()), "arc_fresh": fresh.sum(axis=1).astype(np.int64),
                    "sole": int((fresh.sum(axis=0)[held] == 1).sum()), "held": int(held.sum())})
    return out
