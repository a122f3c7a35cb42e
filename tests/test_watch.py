"""watch.py (CPU): the log of one watched peer from its two byte matrices --
lines, the numbers the other records hold for the peer, and the reference's log
text (Peer.log, Peer.py:40-47, around the entry of Peer.py:206)."""
import datetime

import numpy as np

import raw_csr
import watch_ref

N = 255
# one peer with three in-arcs (senders 7, 2, 7: a repeated arc) and five messages
FIRST = np.array([2, 0, N, 3, 2], np.uint8)             # message 1 was injected at the peer, 2 never came
ARRIVAL = np.array([[2, 1, N, 5, N],
                    [4, N, N, 3, 2],
                    [2, 1, N, 5, N]], np.uint8)
SENDER = np.array([7, 2, 7], np.int32)


def test_lines(pkg):
    ln = pkg.watch.lines(FIRST, ARRIVAL, SENDER)
    got = [(int(x["round"]), int(x["sender"]), int(x["arc"]), int(x["message"]), bool(x["fresh"])) for x in ln]
    assert got == [(1, 7, 0, 1, False), (1, 7, 2, 1, False),           # back to the origin: duplicates
                   (2, 7, 0, 0, True), (2, 2, 1, 4, True), (2, 7, 2, 0, True),
                   (3, 2, 1, 3, True), (4, 2, 1, 0, False), (5, 7, 0, 3, False), (5, 7, 2, 3, False)]
    assert pkg.watch.lines(FIRST, np.empty((0, 5), np.uint8), np.empty(0, np.int32)).size == 0


def test_summary(pkg):
    s = pkg.watch.summary(FIRST, ARRIVAL)
    assert (s["lines"], s["fresh"], s["duplicates"], s["sole"], s["held"]) == (9, 4, 5, 2, 4)
    assert s["arc_lines"].tolist() == [3, 3, 3] and s["arc_fresh"].tolist() == [1, 2, 1]
    assert s["deliverers"].tolist() == [1, 2, 1, 0]                    # injected, one, two, three deliverers
    ref = watch_ref.summaries({"ptr": np.array([0, 3]), "first": FIRST[None, :], "arrival": ARRIVAL})[0]
    assert (ref["lines"], ref["fresh"], ref["sole"], ref["held"]) == (9, 4, 2, 4)
    assert ref["arc_fresh"].tolist() == s["arc_fresh"].tolist()


def test_render_is_the_reference_log_line(pkg):
    peers = [("127.0.0.1", 40001 + k) for k in range(8)]
    origin, inject, count = [3, 0, 1, 5, 3], [0, 0, 0, 2, 1], [1, 1, 1, 2, 2]
    ln = pkg.watch.lines(FIRST, ARRIVAL, SENDER)
    text = pkg.watch.render(ln, peers[0], peers, origin, inject, count)
    assert len(text) == 9
    # Peer.py:398-399 builds the gossip string, Peer.py:206 the entry, Peer.py:42-43 the line -- applied to the same
    # values: round 3, sender peers[2], message 3 (peer 5's second, generated in round 2)
    now = pkg.peer.EPOCH + datetime.timedelta(seconds=3)
    generated = pkg.peer.EPOCH + datetime.timedelta(seconds=2)
    message = f"{generated.strftime('%Y-%m-%d %H:%M:%S')}:{peers[5][0]}:{2}\n"
    peer_addr = peers[2]
    entry = f"[Peer Server] Message from {peer_addr}: {message.strip()}"
    timestamp = now.strftime("%Y-%m-%d %H:%M:%S")
    log_message = f"{timestamp} - {entry}"
    assert text[5] == log_message == "2025-02-22 12:00:03 - [Peer Server] Message from ('127.0.0.1', 40003): " \
                                     "2025-02-22 12:00:02:127.0.0.1:2"
    assert all("\n" not in t for t in text)


def test_arcs_on_a_raw_csr(pkg):
    g = raw_csr.loops_and_repeats(pkg)
    rp, col = np.asarray(g.row_ptr, np.int64), np.asarray(g.col)
    dst = np.repeat(np.arange(g.n), np.diff(rp))
    loop = int(dst[np.nonzero(col == dst)[0][0]])
    verts = [int(np.argmax(np.diff(rp))), loop, 0, g.n - 1]
    ptr, sender = pkg.watch.arcs(g, verts)
    wptr, wsender, _ = watch_ref.arcs(g, verts)
    assert ptr.dtype == np.int64 and sender.dtype == np.int32
    assert np.array_equal(ptr, wptr) and np.array_equal(sender, wsender)
    for s, v in enumerate(verts):
        assert np.array_equal(sender[ptr[s]:ptr[s + 1]], col[rp[v]:rp[v + 1]])     # as loaded: unsorted, repeats kept
    assert loop in sender[ptr[1]:ptr[2]].tolist()
    p0, s0 = pkg.watch.arcs(g, [])
    assert p0.tolist() == [0] and s0.size == 0
