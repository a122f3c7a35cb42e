"""Watched peers (csrc/watch.hip, gp_watch / GP_WATCH_FIRST / GP_WATCH_ARRIVAL)
against tests/watch_ref.py: the arrival log of a list of peers, link by link --
what every reference peer writes line by line (Peer.py:206, Peer.py:286).

The reference of every case is watch_ref.record on the oracle's first-receipt
matrix, never the engine's own outputs; all comparisons are exact.  The watch
set everywhere (watch_set): the highest in-degree vertex, a vertex of in-degree
1, one of in-degree 0 if the overlay has one, vertices 0 and n - 1, one message
origin and 16 random vertices.

Shapes are those of test_gpu_curve / test_gpu_records_matrix: 4,099 and 5
vertices, every row width and the padded ones, the five direction / scan modes,
hubs split at 64 arcs, crashes right after a receipt, churn, a raw CSR, a
directed overlay, every round kind of the pull, message shards, and the C1
bridge.
"""
import functools

import numpy as np
import pytest

import directed_shapes as ds
import raw_csr
import watch_ref
from test_gpu_curve import MODE_IDS, MODES, STAT_KEYS, _width_ref, check_run, mode_cfg, overlay, run
from test_gpu_records_matrix import DNB, DNB_CASES, RECORDS, SPLIT, SPLIT_CASES, _path_ref

pytestmark = pytest.mark.gpu

WIDTH_M = {1: 1, 64: 1, 100: 2, 200: 4, 500: 8, 1000: 16, 2000: 32, 4096: 64, 65: 2, 2049: 64}


def watch_set(g, origin, seed=5):
    deg = np.diff(np.asarray(g.row_ptr, np.int64))
    n = int(g.n)
    picks = [int(np.argmax(deg))]
    for d in (1, 0):
        at = np.nonzero(deg == d)[0]
        if at.size:
            picks.append(int(at[0]))
    picks += [0, n - 1, int(origin[0])]
    picks += np.random.default_rng(seed).choice(n, min(16, n), replace=False).tolist()
    out = []
    for v in picks:
        if v not in out:
            out.append(int(v))
    return out


def watched(pkg, g, origin, inject, verts, records=(), **cfg):
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    for rec in records:
        getattr(eng, "track_" + rec)()
    eng.watch(verts)
    eng.reset()
    return eng


def status(pkg, fn, *args):
    try:
        fn(*args)
    except pkg.GossipError as e:
        return e.status
    return 0


def check_watch(eng, rec, origin=None, inject=None, rounds=None):
    """ptr and both arrays against the reference: the whole run's, or as they
    stand after `rounds` rounds"""
    K, A = len(rec["verts"]), int(rec["ptr"][-1])
    assert eng.watch_info() == (K, A, (A + K) * 64 * eng.words)
    assert np.array_equal(eng.watch_ptr(), rec["ptr"])
    first, arrival = (rec["first"], rec["arrival"]) if rounds is None else watch_ref.after(rec, rounds, origin, inject)
    got_f, got_a = eng.watch_first(), eng.watch_arrival()
    assert got_f.dtype == np.uint8 and got_f.shape == first.shape and got_a.shape == arrival.shape
    assert np.array_equal(got_f, first), np.argwhere(got_f != first)[:8]
    assert np.array_equal(got_a, arrival), np.argwhere(got_a != arrival)[:8]
    for s in (0, K - 1):
        f, a = eng.watch_peer(s)
        assert np.array_equal(f, first[s]) and np.array_equal(a, arrival[rec["ptr"][s]:rec["ptr"][s + 1]])


def check_identities(pkg, eng, g, verts, origin, inject, first=False):
    """the consequences DESIGN.md §2.4 lists per watched peer, on the engine's
    own outputs: load_recv, fresh_recv, link_fresh, sole_recv, seenpop,
    delay_dist and (first) the first-receipt rows"""
    ptr, wf, wa = eng.watch_ptr(), eng.watch_first(), eng.watch_arrival()
    rp = np.asarray(g.row_ptr, np.int64)
    load, fresh, link = eng.load_recv(), eng.fresh_recv(), eng.link_fresh()
    sole, pop, dist = eng.sole_recv(), eng.seenpop(), eng.delay_dist()
    whole = eng.first() if first else None
    inj = np.zeros(eng.m, np.int64) if inject is None else np.asarray(inject, np.int64)
    for s, v in enumerate(verts):
        sm = pkg.watch.summary(wf[s], wa[ptr[s]:ptr[s + 1]])
        assert sm["lines"] == int(load[v]), (s, v)
        assert sm["fresh"] == int(fresh[v]), (s, v)
        assert np.array_equal(sm["arc_fresh"], link[rp[v]:rp[v + 1]].astype(np.int64)), (s, v)
        assert sm["sole"] == int(sole[v]), (s, v)
        assert sm["held"] == int(pop[v]), (s, v)
        held = wf[s] != 255
        delays = np.minimum(wf[s][held].astype(np.int64) - inj[held], 15)
        assert np.array_equal(np.bincount(delays, minlength=16), dist[v].astype(np.int64)), (s, v)
        if whole is not None:
            assert np.array_equal(wf[s], whole[v])
        a = wa[ptr[s]:ptr[s + 1]]
        assert (wf[s][None, :] <= a)[a != 255].all()   # an up receiver holds what it is sent


ALL = RECORDS + ("delay_dist",)


# -- 1. widths and tails ----------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("m", sorted(WIDTH_M))
@pytest.mark.parametrize("n", [4099, 5])
def test_widths_and_tails(pkg, oracle, n, m, mode):
    g, origin, inject, ref = _width_ref(n, m)
    verts = watch_set(g, origin)
    rec = watch_ref.record(g, ref, verts)
    with watched(pkg, g, origin, inject, verts, **mode_cfg(mode)) as eng:
        assert eng.words == WIDTH_M[m]
        stats = run(eng, inject)
        check_watch(eng, rec)
        check_run(eng, stats, ref)
    if n == 4099 and m >= 64:
        assert (rec["arrival"] != 255).any() and (rec["arrival"] != 255).sum() > (rec["first"] != 255).sum()


# -- 2. hubs ------------------------------------------------------------------------

@pytest.mark.parametrize("m", [100, 4096])
def test_hubs_between_rounds(pkg, oracle, m):
    """hub_threshold=64: the watched hub's new rows come from k_hub_final; the
    record is read after every round"""
    g, origin, inject, ref = _width_ref(4099, m)
    assert np.diff(g.row_ptr).max() > 4 * 64
    verts = watch_set(g, origin)
    rec = watch_ref.record(g, ref, verts)
    with watched(pkg, g, origin, inject, verts, hub_threshold=64) as eng:
        stats = []
        for r in range(ref["rounds"]):
            stats.append(eng.round())
            check_watch(eng, rec, origin, inject, r + 1)
        check_watch(eng, rec)
        check_run(eng, stats, ref)


# -- 3. injections and lifecycle ------------------------------------------------------

def test_c1_schedule(pkg, oracle):
    g = overlay(pkg, 4099)
    o, i, _ = pkg.peer.c1_schedule(40, 5, 3)
    origin, inject = np.array(o, np.int32) * 97, np.array(i, np.int32)
    ref = oracle.run(g, origin, inject, want_first=True)
    verts = watch_set(g, origin)
    rec = watch_ref.record(g, ref, verts)
    with watched(pkg, g, origin, inject, verts) as eng:
        stats = []
        for r in range(ref["rounds"]):
            stats.append(eng.round())
            check_watch(eng, rec, origin, inject, r + 1)
        check_run(eng, stats, ref)


def test_lifecycle(pkg, oracle):
    g, origin, inject, ref = _width_ref(4099, 200)
    verts = watch_set(g, origin)
    other = watch_set(g, origin, seed=9)[::-1]
    rec, rec2 = watch_ref.record(g, ref, verts), watch_ref.record(g, ref, other)
    assert not np.array_equal(rec["ptr"], rec2["ptr"])
    with watched(pkg, g, origin, inject, verts) as eng:
        run(eng, inject)
        check_watch(eng, rec)
        a1 = eng.watch_arrival()
        eng.reset()
        assert (eng.watch_arrival() == 255).all() and (eng.watch_first() == 255).all()
        eng.round()
        eng.round()
        check_watch(eng, rec, origin, inject, 2)                  # stopping after 2 rounds
        eng.watch(other)                                          # takes effect at the reset, not before
        check_watch(eng, rec, origin, inject, 2)
        eng.reset()
        run(eng, inject)
        check_watch(eng, rec2)
        eng.watch(verts)
        eng.reset()
        run(eng, inject)
        assert np.array_equal(eng.watch_arrival(), a1)            # two runs after two resets are equal
        eng.watch([])
        check_watch(eng, rec)
        eng.reset()
        assert eng.watch_info() == (0, 0, 0)
        assert status(pkg, eng.watch_first) == pkg._lib.GP_ENOTRACK
        stats = run(eng, inject)
        check_run(eng, stats, ref)


# -- 4. liveness ------------------------------------------------------------------------

def test_crashes_right_after_a_receipt(pkg, oracle):
    g, origin, inject, plain = _width_ref(4099, 200)
    verts = watch_set(g, origin)
    hub = verts[0]
    rp = np.asarray(g.row_ptr, np.int64)
    got2 = [v for v in verts[1:] if (plain["first"][v] == 2).any()][:3]          # watched peers that receive in round 1
    senders = [int(u) for u in np.asarray(g.col)[rp[hub]:rp[hub + 1]] if (plain["first"][u] == 2).any()][:5]
    assert got2 and senders
    crashes = sorted({(v, 2) for v in got2} | {(u, 2) for u in senders if u != hub})
    ref = oracle.run(g, origin, inject, crashes=crashes, want_first=True)
    rec = watch_ref.record(g, ref, verts, crashes=crashes)
    base = watch_ref.record(g, plain, verts)
    assert (rec["arrival"] != 255).sum() < (base["arrival"] != 255).sum()
    with watched(pkg, g, origin, inject, verts, hub_threshold=64) as eng:
        by_round = {2: [v for v, _ in crashes]}
        stats = []
        for r in range(ref["rounds"]):
            if r in by_round:
                eng.crash(by_round[r])
            stats.append(eng.round())
            check_watch(eng, rec, origin, inject, r + 1)
        check_run(eng, stats, ref)


@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[4]], ids=["pull", "push", "adaptive"])
def test_churn(pkg, oracle, mode):
    g, origin, inject, _ = _width_ref(4099, 200)
    kw = dict(churn=True, p_fail=0.01, churn_seed=11)
    ref = oracle.run(g, origin, inject, want_first=True, **kw)
    assert sum(s["crashed"] for s in ref["stats"]) > 0 and sum(s["removals"] for s in ref["stats"]) > 0
    verts = watch_set(g, origin)
    rec = watch_ref.record(g, ref, verts, **kw)
    with watched(pkg, g, origin, inject, verts, churn=1, p_fail=0.01, churn_seed=11, **mode_cfg(mode)) as eng:
        stats = run(eng, inject)
        check_watch(eng, rec)
        check_run(eng, stats, ref)


# -- 5. raw CSR and directed overlay -------------------------------------------------------

def test_raw_csr(pkg, oracle):
    g = raw_csr.loops_and_repeats(pkg)
    m = 100
    origin = pkg.overlay.random_origins(g.n, m, seed=41)
    inject = (np.arange(m) % 3).astype(np.int32)
    ref = oracle.run(g, origin, inject, want_first=True)
    rp, col = np.asarray(g.row_ptr, np.int64), np.asarray(g.col, np.int64)
    dst = np.repeat(np.arange(g.n), np.diff(rp))
    loop = int(dst[np.nonzero(col == dst)[0][0]])
    twin = next(int(v) for v in range(g.n) if np.unique(col[rp[v]:rp[v + 1]]).size < rp[v + 1] - rp[v] and v != loop)
    verts = [v for v in watch_set(g, origin) if v not in (loop, twin)] + [loop, twin]
    rec = watch_ref.record(g, ref, verts)
    s = len(verts) - 2
    a = rec["arrival"][rec["ptr"][s]:rec["ptr"][s + 1]]
    me = rec["sender"][rec["ptr"][s]:rec["ptr"][s + 1]] == loop
    held = rec["first"][s] != 255
    assert held.any() and (a[me][:, held] == rec["first"][s][held] + 1).all()       # a self-loop: a row of duplicates
    a = rec["arrival"][rec["ptr"][s + 1]:rec["ptr"][s + 2]]
    u = rec["sender"][rec["ptr"][s + 1]:rec["ptr"][s + 2]]
    same = [np.nonzero(u == x)[0] for x in np.unique(u) if (u == x).sum() > 1]
    assert same and all(np.array_equal(a[i[0]], a[i[1]]) for i in same)           # a repeated arc: two equal rows
    with watched(pkg, g, origin, inject, verts, ALL, hub_threshold=64) as eng:
        stats = run(eng, inject)
        check_watch(eng, rec)
        check_identities(pkg, eng, g, verts, origin, inject)
        check_run(eng, stats, ref)


def test_directed(pkg, oracle):
    g = ds.oriented_chung_lu(pkg, oracle, 4099, 8, 2.2, 5, "coin")
    assert g.directed
    m = 200
    origin = pkg.overlay.random_origins(g.n, m, seed=2)
    inject = (np.arange(m) % 3).astype(np.int32)
    ref = oracle.run(g, origin, inject, want_first=True)
    verts = watch_set(g, origin)
    rec = watch_ref.record(g, ref, verts)
    assert (rec["arrival"] != 255).any()
    with watched(pkg, g, origin, inject, verts, ALL) as eng:
        stats = run(eng, inject)
        check_watch(eng, rec)
        check_identities(pkg, eng, g, verts, origin, inject)
        check_run(eng, stats, ref)


# -- 6. commit paths, the watch beside the seven records ------------------------------------

def _scans(stats):
    return [s["scan"] for s in stats]


PATHS = {
    "compact-rec": ((4099, 8, 2.5, 31, 2049, None),
                    dict(push_ratio=0.0, prefilter_pct=0, arc_mask_permille=0, compact_rows=1, hub_threshold=1 << 30), 64,
                    lambda st: any((s["scan"] & 3) == 0 and s["scan"] & 4 for s in st)),
    "compact-pre": ((65584, 8, 2.5, 31, 2049, None),
                    dict(push_ratio=0.0, prefilter_pct=20, arc_mask_permille=0, compact_rows=1, hub_threshold=1 << 30), 64,
                    lambda st: any((s["scan"] & 3) == 3 and s["scan"] & 4 for s in st)),
    "sated-churn": ((4099, 12, 2.4, 31, 2049, None, (0.02, 7)),
                    dict(hub_threshold=256, push_ratio=0.0, unfiltered_pct=0, flat_max_words=0, arc_mask_permille=0), 64,
                    lambda st: sum(s["crashed"] for s in st) > 0 and sum(s["done_nb"] for s in st) > 0),
    "aliases-lists": ((120_000, 12, 2.4, 41, 4096, None, None),
                      dict(push_ratio=0.0, unfiltered_pct=0, hub_threshold=1 << 30, arc_mask_permille=0, compact_rows=0), 64,
                      lambda st: sum(s["aliased"] for s in st) > 0 and any(s["scan"] & 64 for s in st)),
}
for _k, (_seed, _m, _cfg, _w) in DNB_CASES.items():
    PATHS["dnb-" + _k] = ((4099, 12, 2.5, _seed, _m, None), _cfg, _w, lambda st: sum(s["done_nb"] for s in st) > 0)
for _k in ("W64", "W32", "W8-receiver"):
    _n, _m, _f, _w = SPLIT_CASES[_k]
    PATHS["split-" + _k] = ((_n, 10, 2.4, 61, _m, 2), dict(SPLIT, flat_max_words=_f), _w,
                            lambda st: any(x & 32 for x in _scans(st)))


def path_run(pkg, shape, cfg):
    g, origin, inject, kw, ref = _path_ref(*shape)
    verts = watch_set(g, origin)
    rec = watch_ref.record(g, ref, verts, **kw)
    if kw:
        cfg = dict(cfg, churn=1, p_fail=kw["p_fail"], churn_seed=kw["churn_seed"])
    small = g.n * len(origin) <= 1 << 26
    with watched(pkg, g, origin, inject, verts, ALL, track_first=1 if small else 0, **cfg) as eng:
        stats = run(eng, inject)
        check_watch(eng, rec)
        check_identities(pkg, eng, g, verts, origin, inject, first=small)
        check_run(eng, stats, ref)
        return stats, eng.words


@pytest.mark.parametrize("case", list(PATHS))
def test_commit_paths(pkg, oracle, case):
    """one case per round kind of test_gpu_records_matrix part C, its own
    round-kind assertion kept: a commit path that stored a stale or partial
    frontier row would leave seen and digest right and the log wrong"""
    shape, cfg, words, kind = PATHS[case]
    stats, W = path_run(pkg, shape, cfg)
    assert W == words
    assert kind(stats), _scans(stats)


def test_line_done_pack(pkg, oracle, monkeypatch):
    shape = (4099, 8, 2.5, 5, 2049, None)
    cfg = dict(push_ratio=0.0, unfiltered_pct=1, hub_threshold=1 << 30)
    monkeypatch.setenv("GP_LINE_DONE_MIN_DEG", "16")
    runs = {}
    for v in ("1", "0"):
        monkeypatch.setenv("GP_LINE_DONE", v)
        monkeypatch.setenv("GP_LINE_PACK", v)
        runs[v], W = path_run(pkg, shape, cfg)
        assert W == 64
    moved = [a["round"] for a, b in zip(runs["1"], runs["0"])
             if a["scan"] == 2 and (a["rows_gathered"], a["row_bytes"]) != (b["rows_gathered"], b["row_bytes"])]
    assert moved, "no unfiltered round's row_bytes or rows_gathered moved"


# -- 7. shards ----------------------------------------------------------------------------

def test_message_shards(pkg, oracle):
    g, origin, inject, ref = _width_ref(4099, 4096)
    verts = watch_set(g, origin)
    rec = watch_ref.record(g, ref, verts)
    cuts = [0, 256, 768, 2816, 4096]
    firsts, arrivals = [], []
    for (lo, hi), words in zip(zip(cuts[:-1], cuts[1:]), (4, 8, 32, 32)):
        with pkg.GossipEngine(0) as eng:
            eng.load_graph(g)
            eng.set_message_shard(origin, inject, lo, hi)
            eng.watch(verts)
            eng.reset()
            assert eng.words == words
            run(eng, inject[lo:hi])
            assert np.array_equal(eng.watch_ptr(), rec["ptr"])
            firsts.append(eng.watch_first())
            arrivals.append(eng.watch_arrival())
    assert np.array_equal(np.concatenate(firsts, axis=1), rec["first"])
    assert np.array_equal(np.concatenate(arrivals, axis=1), rec["arrival"])


# -- 8. neutrality ----------------------------------------------------------------------------

READS = ("digest", "first", "curve", "load_sent", "load_recv", "fresh_sent", "fresh_recv", "fresh_curve", "link_fresh",
         "delay_sum", "delay_max", "sole_sent", "sole_recv", "mult_hist", "delay_dist", "seenpop")


@pytest.mark.parametrize("mode", [MODES[0], MODES[4]], ids=["pull", "adaptive"])
def test_watching_changes_no_other_output(pkg, oracle, mode):
    g, origin, inject, ref = _width_ref(4099, 200)
    outs = []
    for verts in (watch_set(g, origin), []):
        with watched(pkg, g, origin, inject, verts, ALL, track_first=1, hub_threshold=64, **mode_cfg(mode)) as eng:
            stats = run(eng, inject)
            outs.append((stats, {k: getattr(eng, k)() for k in READS}))
            check_run(eng, stats, ref)
    (sa, ra), (sb, rb) = outs
    keep = STAT_KEYS + ("mode", "scan", "arcs_scanned", "rows_gathered", "rows_written")
    assert [[s[k] for k in keep] for s in sa] == [[s[k] for k in keep] for s in sb]
    for k in READS:
        assert np.array_equal(ra[k], rb[k]), k
    assert np.array_equal(ra["first"], ref["first"])


# -- 9. errors ----------------------------------------------------------------------------------

def test_errors(pkg, oracle):
    lib = pkg._lib
    g, origin, inject, ref = _width_ref(4099, 200)
    verts = watch_set(g, origin)
    rec = watch_ref.record(g, ref, verts)
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, inject)
        eng.reset()
        assert eng.watch_info() == (0, 0, 0)
        assert status(pkg, eng.watch_first) == lib.GP_ENOTRACK
        assert status(pkg, eng.watch, [0, g.n]) == lib.GP_EINVAL
        assert status(pkg, eng.watch, [-1]) == lib.GP_EINVAL
        assert status(pkg, eng.watch, [3, 7, 3]) == lib.GP_EINVAL
        eng.watch(verts)
        assert status(pkg, eng.watch_arrival) == lib.GP_ENOTRACK                # before the reset
        assert status(pkg, eng.watch_peer, 0) == lib.GP_ENOTRACK
        eng.reset()
        need = (int(g.nnz) + g.n) * 64 * eng.words                              # every vertex watched
        everyone = verts + [v for v in range(g.n) if v not in verts]
        try:
            eng.watch(everyone, max_bytes=need - 1)
            raise AssertionError("over budget, accepted")
        except pkg.GossipError as e:
            assert e.status == lib.GP_ENOMEM and str((int(g.nnz) + g.n) * 64 * eng.words) in str(e), str(e)
        eng.watch(everyone, max_bytes=need)                                     # (exactly enough is accepted)
        eng.watch(verts)
        assert status(pkg, eng.watch, everyone, need - 1) == lib.GP_ENOMEM
        eng.reset()                                                             # the previous list is still in force
        run(eng, inject)
        check_watch(eng, rec)
        K, A = len(verts), int(rec["ptr"][-1])
        fn = eng._lib.gp_read
        buf = np.full(K * eng.m + 1, 77, np.uint8)
        assert fn(eng._ctx, lib.WATCH_FIRST, buf.ctypes.data, K * eng.m + 1) == lib.GP_EINVAL and (buf == 77).all()
        assert fn(eng._ctx, lib.WATCH_ARRIVAL, buf.ctypes.data, A * eng.m - 1) == lib.GP_EINVAL
        assert fn(eng._ctx, lib.WATCH_PTR, buf.ctypes.data, K * 8) == lib.GP_EINVAL
        assert status(pkg, eng.watch_peer, K) == lib.GP_EINVAL and status(pkg, eng.watch_peer, -1) == lib.GP_EINVAL
        rd = eng._lib.gp_read_watch_peer
        assert rd(eng._ctx, 0, buf.ctypes.data, buf.ctypes.data, 1) == lib.GP_EINVAL
        eng.reset()
        eng.round()
        eng.round()
        blob = eng.checkpoint()
        with watched(pkg, g, origin, inject, verts) as other:
            other.restore(blob)
            assert status(pkg, other.watch_first) == lib.GP_ESTATE
            assert status(pkg, other.watch_peer, 0) == lib.GP_ESTATE
            run(other, inject)
            assert status(pkg, other.watch_arrival) == lib.GP_ESTATE
            other.reset()
            run(other, inject)
            check_watch(other, rec)
    with pkg.GossipEngine(0) as eng:
        eng.load_graph(g)
        eng.set_partition(0, 2)
        eng.set_messages(origin, inject)
        eng.watch(verts)
        eng.reset()
        assert status(pkg, eng.watch_first) == lib.GP_ENOTRACK
        assert status(pkg, eng.watch_peer, 0) == lib.GP_ENOTRACK


# -- 10. bridge ------------------------------------------------------------------------------------

def test_bridge(pkg, oracle):
    def bridge(**cfg):
        b = pkg.bridge.ProtocolBridge(**cfg)
        for k in range(12):
            b.handle(str(("127.0.0.1", 40001 + k)) + "\n")
        b.start()
        return b
    who = [("127.0.0.1", 40001 + k) for k in (3, 0, 11)]
    crash_at, victim = 6, ("127.0.0.1", 40001 + 2)
    wb, pb = bridge(watch=who), bridge()
    g = wb.overlay()
    verts = [wb.vertex[w] for w in who]
    ref = oracle.run(g, wb.origin, wb.inject, crashes=[(wb.vertex[victim], crash_at)], want_first=True)
    rec = watch_ref.record(g, ref, verts, crashes=[(wb.vertex[victim], crash_at)])
    total = 0
    for r in range(ref["rounds"]):
        if r == crash_at:
            wb.crash(victim)
            pb.crash(victim)
        a, b = wb.step(), pb.step()
        assert "arrivals" not in b
        assert sorted(a["deliveries"]) == sorted(d for d in b["deliveries"] if d[0] in who)
        want = [(who[rec["slot"][x]], wb.peers[int(rec["sender"][x])], wb.gossip_line(k),
                 bool(rec["arrival"][x, k] == rec["first"][rec["slot"][x], k]))
                for x, k in np.argwhere(rec["arrival"] == r + 1).tolist()]
        assert sorted(a["arrivals"]) == sorted(want)
        total += len(want)
    assert total == int((rec["arrival"] != 255).sum()) > 0
    assert wb.engine.cfg.track_first == 0
    wb.close()
    pb.close()
