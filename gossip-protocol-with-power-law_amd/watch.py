"""Watched peers: host helpers for the arrival log of chosen peers
(csrc/watch.hip).  numpy only, no engine inside.

The reference's user-facing output is a log per peer: every gossip line that
arrives is written down with the peer it came from and the time (Peer.py:206,
Peer.py:286, through Peer.log, Peer.py:40-47).  GossipEngine.watch() keeps that
log for a list of peers as two byte matrices -- watch_first u8 [K][m] and
watch_arrival u8 [A][m], the receipt round per (in-arc, message), 255 = never
-- and the functions here turn one peer's share of them (GossipEngine.
watch_peer) back into lines, into the numbers the other records hold for that
peer, and into the reference's log text.
"""
import numpy as np

from . import peer as wire

NEVER = 255
LINE = np.dtype([("round", np.uint8), ("sender", np.int32), ("arc", np.int64), ("message", np.int32),
                 ("fresh", np.bool_)])


def arcs(graph, verts):
    """(ptr i64 [K + 1], sender i32 [A]): watched arc ptr[s] + i is the i-th
    arc of row verts[s] of the in-CSR `graph` (row_ptr, col) as loaded -- a raw
    CSR's parallel arcs and self-loops included -- and sender[a] the peer it
    comes from.  ptr is GossipEngine.watch_ptr()."""
    rp = np.asarray(graph.row_ptr, np.int64)
    col = np.asarray(graph.col, np.int32)
    v = np.asarray(verts, np.int64).reshape(-1)
    ptr = np.concatenate([[0], np.cumsum(rp[v + 1] - rp[v])]).astype(np.int64)
    sender = np.concatenate([col[rp[x]:rp[x + 1]] for x in v.tolist()] + [np.empty(0, np.int32)]).astype(np.int32)
    return ptr, sender


def _check(first_row, arrival):
    first_row = np.asarray(first_row, np.uint8).reshape(-1)
    arrival = np.asarray(arrival, np.uint8).reshape(-1, first_row.size)
    return first_row, arrival


def lines(first_row, arrival, sender):
    """The log of one peer: a structured array (round, sender, arc, message,
    fresh), one entry per arrival, sorted by (round, arc, message).  `arc` is
    the arc's index in the peer's in-list, `sender` the peer at its other end
    (sender[arc]), `round` the receipt round, and `fresh` says whether the line
    told the peer something it did not hold (round == first_row[message])."""
    first_row, arrival = _check(first_row, arrival)
    sender = np.asarray(sender, np.int32).reshape(-1)
    if sender.size != arrival.shape[0]:
        raise ValueError("one sender per arc of the arrival matrix")
    a, k = np.nonzero(arrival != NEVER)
    rr = arrival[a, k]
    order = np.lexsort((k, a, rr))
    out = np.empty(order.size, LINE)
    out["round"] = rr[order]
    out["arc"] = a[order]
    out["message"] = k[order]
    out["sender"] = sender[a[order]]
    out["fresh"] = rr[order] == first_row[k[order]]
    return out


def summary(first_row, arrival):
    """The numbers the other records hold for this peer, from its log alone:
      lines, fresh, duplicates     load_recv[v], fresh_recv[v], their difference
      arc_lines, arc_fresh         int64 [deg]: per in-arc; arc_fresh is link_fresh
      deliverers                   int64 [deg + 1]: messages the peer holds by the
                                   number of arcs that delivered them fresh (index 0:
                                   injected at the peer)
      sole                         messages with exactly one fresh arc: sole_recv[v]
      held                         messages the peer holds: seenpop[v]
    """
    first_row, arrival = _check(first_row, arrival)
    got = arrival != NEVER
    fresh = got & (arrival == first_row[None, :])
    per_msg = fresh.sum(axis=0)
    held = first_row != NEVER
    return {"lines": int(got.sum()), "fresh": int(fresh.sum()), "duplicates": int(got.sum() - fresh.sum()),
            "arc_lines": got.sum(axis=1).astype(np.int64), "arc_fresh": fresh.sum(axis=1).astype(np.int64),
            "deliverers": np.bincount(per_msg[held], minlength=arrival.shape[0] + 1).astype(np.int64),
            "sole": int((per_msg[held] == 1).sum()), "held": int(held.sum())}


def render(lines, to, peers, origin, inject, count):
    """The reference's log text for the peer with identity `to`, one line per
    arrival in log order:

      "{timestamp} - [Peer Server] Message from {peers[sender]}: {gossip line}"

    the format of Peer.log (Peer.py:43) around the entry of Peer.py:206, with
    timestamp = peer.timestamp(peer.round_time(round)) and the gossip line
    peer.gossip_message(round_time(inject[k]), ip of peers[origin[k]],
    count[k]), stripped as Peer.py:206 strips it.  The reference prints the
    connecting socket's ephemeral address where this prints the sender's
    identity (ip, port) -- the bridge's convention: a peer is named by the
    address it registered.  `to` names whose log this is (the reference writes
    peer_log_{port}.txt, Peer.py:37); it is not part of a line."""
    del to
    out = []
    for ln in lines:
        k = int(ln["message"])
        gossip = wire.gossip_message(wire.round_time(int(inject[k])), peers[int(origin[k])][0], int(count[k])).strip()
        out.append(f"{wire.timestamp(wire.round_time(int(ln['round'])))} - [Peer Server] Message from "
                   f"{tuple(peers[int(ln['sender'])])}: {gossip}")
    return out
