"""The packed row gather of the W = 64 early-exit pulls (DESIGN.md §3.3,
csrc/line_pack.h, gather_rows_pack): GP_LINE_PACK=1 against =0, and both
against the CPU oracle.

The packed gather only deals the lanes of the serial loop's row loads out over
the 128-B lines a receiver still misses: eight or four senders' rows per
wave-instruction instead of two.  OR is idempotent, so every output and every
protocol counter -- the reference's send loop over every link (Peer.py:402-404)
and its Message-List dedup (Peer.py:175-216) -- must stay bit for bit what the
oracle computes; only rows_gathered and row_bytes may move, in either
direction (a packed batch holds more rows past an early exit, and fewer
batches run).

Shape, helpers and references are those of tests/test_gpu_line_done.py:
Chung-Lu 200,000 x mean degree 8, gamma 2.5, 4096 messages in spread order,
every round a pull, unfiltered from 1 % senders, no hubs unless a case says so.
The default gate needs more than 2^19 vertices; tests/test_full_size.py runs
the bench configuration there.
"""
import numpy as np
import pytest

import test_gpu_line_done as ld

pytestmark = pytest.mark.gpu

M = ld.M
STAT_KEYS = ld.STAT_KEYS


def _run(pkg, monkeypatch, g, origin, inject, pack, line_done=0, **kw):
    """ld._run with GP_LINE_PACK set as given (None: unset) at gp_create."""
    if pack is None:
        monkeypatch.delenv("GP_LINE_PACK", raising=False)
    else:
        monkeypatch.setenv("GP_LINE_PACK", str(pack))
    return ld._run(pkg, monkeypatch, g, origin, inject, line_done=line_done, **kw)


def _check_on_off(on, off, work=True):
    """Same protocol, same outputs, same commits; the gather's two work
    counters differ in at least one round (the packed path ran)."""
    print("on :", ld._work(on))
    print("off:", ld._work(off))
    assert len(on["stats"]) == len(off["stats"])
    moved = False
    for a, b in zip(on["stats"], off["stats"]):
        for k in STAT_KEYS + ("mode", "scan"):
            assert a[k] == b[k], (k, a["round"])
        if work:
            assert a["done_nb"] == b["done_nb"], a["round"]
            assert a["rows_written"] + a["aliased"] == b["rows_written"] + b["aliased"], a["round"]
            assert a["arcs_scanned"] == b["arcs_scanned"], a["round"]
            assert a["row_bytes"] <= 8 * 64 * a["rows_gathered"], a["round"]
            moved = moved or a["row_bytes"] != b["row_bytes"] or a["rows_gathered"] != b["rows_gathered"]
    for k in ("seen", "digest", "coverage", "forwards"):
        assert np.array_equal(on[k], off[k]), k
    if work:
        assert moved, "no round's row_bytes or rows_gathered moved: the packed gather did not run"


@pytest.fixture(scope="module")
def base(pkg, oracle):
    g = ld._overlay(pkg, oracle, "one")
    origin, inject = ld._messages(pkg, g)
    return g, origin, inject, ld._reference(oracle, "one", g, origin, inject)


@pytest.mark.parametrize("line_done", [0, 1])
def test_on_against_off_to_quiescence(pkg, base, monkeypatch, line_done):
    """Packed against row layout, the per-line done-neighbour rule forced off
    and on: both to quiescence, both equal to the oracle."""
    g, origin, inject, ref = base
    on = _run(pkg, monkeypatch, g, origin, inject, pack=1, line_done=line_done)
    off = _run(pkg, monkeypatch, g, origin, inject, pack=0, line_done=line_done)
    ld._check_oracle(on, ref)
    ld._check_oracle(off, ref)
    _check_on_off(on, off)
    # the plain early-exit pull (before any receiver aliases) ran packed; the
    # near-done pulls behind it keep the parent's gather
    moved = [(a["aliased"] > 0) for a, b in zip(on["stats"], off["stats"])
             if a["scan"] == 2 and (a["rows_gathered"], a["row_bytes"]) != (b["rows_gathered"], b["row_bytes"])]
    assert moved and True not in moved, moved


def test_default_gate_is_off_at_this_size(pkg, base, monkeypatch):
    """No override: 200,000 x 512 B stay inside the Infinity Cache, the parent's gather runs."""
    g, origin, inject, ref = base
    dflt = _run(pkg, monkeypatch, g, origin, inject, pack=None, line_done=None, min_deg=None)
    off = _run(pkg, monkeypatch, g, origin, inject, pack=0, line_done=None, min_deg=None)
    ld._check_oracle(dflt, ref)
    ld._same_work(dflt, off)


def test_staggered_injection(pkg, base, oracle, monkeypatch):
    """Inject rounds 0-2: the lines fill in another order, and targets grow between rounds."""
    g = base[0]
    origin, inject = ld._messages(pkg, g, staggered=True)
    ref = ld._reference(oracle, "staggered", g, origin, inject)
    on = _run(pkg, monkeypatch, g, origin, inject, pack=1)
    off = _run(pkg, monkeypatch, g, origin, inject, pack=0)
    ld._check_oracle(on, ref)
    _check_on_off(on, off)


def test_two_components(pkg, oracle, monkeypatch):
    """Two components, messages in both: a receiver's dead lines include those
    on which its component has no message at all."""
    g = ld._overlay(pkg, oracle, "two")
    origin, inject = ld._messages(pkg, g)
    ref = ld._reference(oracle, "two", g, origin, inject)
    on = _run(pkg, monkeypatch, g, origin, inject, pack=1)
    off = _run(pkg, monkeypatch, g, origin, inject, pack=0)
    ld._check_oracle(on, ref)
    _check_on_off(on, off)


def test_reset_and_second_run(pkg, base, monkeypatch):
    """A second run in the same context: equal outputs and equal work (the
    parked rows in LDS carry nothing from receiver to receiver or run to run)."""
    g, origin, inject, ref = base
    first, second = _run(pkg, monkeypatch, g, origin, inject, pack=1, runs=2)
    ld._check_oracle(first, ref)
    ld._check_oracle(second, ref)
    ld._same_work(first, second)


def test_hub_splits_on(pkg, base, monkeypatch):
    """hub_threshold 64: the hub chunks run beside the packed main kernel and
    keep the row layout.  Outputs only (their work counters depend on wave timing)."""
    g, origin, inject, ref = base
    assert np.diff(g.row_ptr).max() > 64
    on = _run(pkg, monkeypatch, g, origin, inject, pack=1, hub_threshold=64)
    ld._check_oracle(on, ref)


# ---------------------------------------------------------------------------
# A crafted overlay: receivers whose in-degrees straddle every batch edge, in
# every live-line state the layout distinguishes.
#
# Line l is messages [1024 l, 1024 l + 1024).  Two of them per line are
# "special": one in the first and one in the last word of the line.
#   X_l  64 origins of line l's 1022 other messages       (hold them in round 0)
#   O_l  the origin of line l's two special messages
#   H_l  hub of X_l and O_l: all of line l from round 1
#   G_l  hub of X_l only: line l without the special bits from round 1
#   Y_l  neighbour of O_l: the special bits of line l from round 1
#   B    bulk vertices under all four H: they take the whole table in round 1,
#        which makes round 2 an early-exit round with under half the bits held
# A receiver hangs under H_l for the lines it is to hold already (from round
# 1), under fillers that hang under some H / G (a line, with or without its
# special bits, from round 1; two pad leaves each keep them ahead in the gather
# order), and under one last sender Z that hangs under Y_l only: the special
# bits of the lines still missing, from round 1, held by nobody else the
# receiver sees.  Round 2 is the round the receivers gather in.
SPECIAL = (5, 1023 - 5)
DEGREES = (1, 2, 3, 4, 5, 8, 9, 12, 13, 24, 25, 32, 33, 64, 65, 100)


def _specs():
    """(held lines, fillers [(lines, with special bits)], Z's lines) per receiver."""
    def one(l, d):      # exactly one live line
        return [x for x in range(4) if x != l], [((l,), False)] * (d - 4), (l,)

    def two(p, q, d):   # two live lines
        return [x for x in range(4) if x not in (p, q)], [((p, q), False)] * (d - 3), (p, q)

    def cascade(d):     # 4 -> 2 -> 1: lines 0-1 in the first batch, line 2 in the next, line 3 last
        return [], [((0, 1), True)] * 6 + [((2,), True)] * 4 + [((3,), False)] * (d - 11), (3,)

    s = {1: [([], [], (0,))], 2: [([1], [], (2,))], 3: [two(0, 3, 3)], 4: [one(l, 4) for l in range(4)],
         5: [one(1, 5), two(1, 2, 5)], 8: [one(2, 8), two(0, 3, 8)], 9: [one(3, 9), two(2, 3, 9)],
         12: [two(1, 2, 12), cascade(12), one(0, 12)], 13: [cascade(13), one(1, 13), two(0, 3, 13)],
         24: [one(3, 24), cascade(24), two(0, 1, 24)], 25: [cascade(25), one(2, 25), two(0, 3, 25)],
         32: [two(0, 3, 32), one(0, 32), cascade(32)], 33: [one(0, 33), two(1, 2, 33), cascade(33)],
         64: [cascade(64), one(1, 64), two(0, 3, 64)], 65: [one(2, 65), two(1, 2, 65), cascade(65)],
         100: [cascade(100), one(3, 100), two(0, 3, 100)]}
    assert tuple(sorted(s)) == DEGREES
    return [(d, spec) for d in DEGREES for spec in s[d]]


def _crafted(pkg):
    edges, recv = [], []
    nxt = [0]

    def new(k=1):
        v = np.arange(nxt[0], nxt[0] + k)
        nxt[0] += k
        return v

    H, G, Y, O = new(4), new(4), new(4), new(4)
    X = [new(64) for _ in range(4)]
    for l in range(4):
        edges += [(H[l], x) for x in X[l]] + [(G[l], x) for x in X[l]] + [(H[l], O[l]), (Y[l], O[l])]
    for d, (held, fillers, zl) in _specs():
        r = int(new()[0])
        edges += [(H[l], r) for l in held]
        for lines, full in fillers:
            f = int(new()[0])
            edges += [((H if full else G)[l], f) for l in lines] + [(f, r)] + [(f, int(p)) for p in new(2)]
        z = int(new()[0])
        edges += [(Y[l], z) for l in zl] + [(z, r)]
        assert len(held) + len(fillers) + 1 == d
        recv.append((r, d, z, zl))
    bulk = new(nxt[0] // 3)
    edges += [(H[l], int(b)) for l in range(4) for b in bulk]
    g = pkg.CSR.from_edges(nxt[0], np.array(edges, np.int64))
    origin = np.empty(M, np.int32)
    for k in range(M):
        l, j = divmod(k, 1024)
        origin[k] = O[l] if j in SPECIAL else X[l][j % 64]
    return g, origin, recv


def _line_masks(bits):
    """[4096] bool -> 4-bit mask of the lines holding a set bit."""
    return sum(1 << l for l in range(4) if bits[1024 * l:1024 * (l + 1)].any())


def _walk(want, rows, rif=3):
    """The packed serial loop on the CPU: the live-line mask at every batch."""
    acc = np.zeros(M, bool)
    masks, k0 = [], 0
    while k0 < len(rows):
        lm = _line_masks(want & ~acc)
        if not lm:
            break
        masks.append(lm)
        p = bin(lm).count("1")
        nb = rif * (8 if p == 1 else 4 if p == 2 else 2)
        acc |= rows[k0:k0 + nb].any(0)
        k0 += nb
    return masks, bool((want & ~acc).any())


def test_crafted_states(pkg, oracle, monkeypatch):
    g, origin, recv = _crafted(pkg)
    assert g.n < 20_000
    ref = oracle.run(g, origin, None, nthreads=16, want_first=True)
    first = ref["first"]
    nm = g.n * M
    held = np.cumsum([s["new_bits"] + s["injected"] for s in ref["stats"]])
    # round 2: early exit (round 1's receipts), under half the bits held (the plain pull), 1 % senders
    assert ref["stats"][1]["new_bits"] * 16 >= nm and held[1] * 2 < nm
    deg = np.diff(g.row_ptr)
    assert sorted(set(int(deg[r]) for r, *_ in recv)) == list(DEGREES)
    seen_masks, seqs, last_only = set(), [], 0
    for r, d, z, zl in recv:
        assert deg[r] == d
        nb = g.col[g.row_ptr[r]:g.row_ptr[r + 1]]
        nb = nb[np.lexsort((nb, -deg[nb]))]   # gather order: in-degree descending, ties by id
        want = (first[r] != 255) & ~(first[r] <= 2)
        rows = first[nb] <= 2
        assert want.any(), (r, d)
        masks, left = _walk(want, rows)
        seen_masks.update(masks)
        seqs.append(masks)
        # the special bits of Z's lines: held by the last arc alone, in the first and last word of the line
        assert nb[-1] == z
        for l in zl:
            for j in SPECIAL:
                k = 1024 * l + j
                assert want[k] and rows[-1, k] and not rows[:-1, k].any(), (r, d, k)
                assert k // 64 in (16 * l, 16 * l + 15)
            last_only += 1
    pop = [bin(m).count("1") for m in range(16)]
    assert {1, 2, 4, 8} <= seen_masks, seen_masks                       # one live line, each of the four
    assert 0b1001 in seen_masks and {0b0110, 0b0011, 0b1100} & seen_masks, seen_masks   # two: apart, adjacent
    assert any(any(pop[a] == 4 and pop[b] == 2 and pop[c] == 1 for a, b, c in zip(s, s[1:], s[2:])) for s in seqs), \
        "no receiver moves 4 -> 2 -> 1 inside one gather"
    assert any(len(s) >= 2 and d > 64 for s, (_, d, _, _) in zip(seqs, recv))   # a second pass in packed state
    assert last_only >= len(recv)
    for a in ("seen", "digest", "coverage", "forwards"):
        ref[a].setflags(write=False)
    on = _run(pkg, monkeypatch, g, origin, None, pack=1)
    off = _run(pkg, monkeypatch, g, origin, None, pack=0)
    ld._check_oracle(on, ref)
    ld._check_oracle(off, ref)
    _check_on_off(on, off)
    a2, b2 = on["stats"][2], off["stats"][2]
    assert a2["scan"] == 2 and a2["aliased"] == 0 and a2["done_nb"] == 0   # the plain early-exit pull
    assert (a2["rows_gathered"], a2["row_bytes"]) != (b2["rows_gathered"], b2["row_bytes"])
