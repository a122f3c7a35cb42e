"""The lifecycle every per-run record shares (csrc/records.h):
asked for by its gp_track_* call (gp_watch), in force from the next gp_reset,
lost by a checkpoint restored past round 0, refused by lossy and delayed links
where it walks arcs, and kept by a vertex-partitioned context or not.

One tiny shape per case: a Barabasi-Albert overlay of 300 vertices with 70
messages (W = 2) injected in rounds 0 and 1, so that the receipt delays and
their distributions read the frontier rows; those two also run 40 messages
(W = 1) injected in round 0, the pass over the per-vertex counts alone.  Every
check is a host-side status code or an exact comparison of the engine with
itself: a run that keeps one record reads what the run that keeps all nine
reads.  The records' values against their references -- the aggregates of what
each reference peer logs per arrival (Peer.py:175-216) -- are the subject of
the records' own test files.
"""
import functools

import numpy as np
import pytest

from test_gpu_curve import run

pytestmark = pytest.mark.gpu

N, BA_M, SEED = 300, 3, 11
WATCHED = [0, 7, 150, 299]   # vertex 0: the hub of the attachment process


def _on(name):
    return lambda e: getattr(e, name)()


def _off(name):
    return lambda e: getattr(e, name)(False)


# name -> (turn on, turn off, the reads)
RECORDS = {
    "load": (_on("track_load"), _off("track_load"), ("load_sent", "load_recv")),
    "curve": (_on("track_curve"), _off("track_curve"), ("curve",)),
    "fresh": (_on("track_fresh"), _off("track_fresh"), ("fresh_sent", "fresh_recv")),
    "mult": (_on("track_mult"), _off("track_mult"), ("sole_sent", "sole_recv", "mult_hist", "sole_bins")),
    "fresh_curve": (_on("track_fresh_curve"), _off("track_fresh_curve"), ("fresh_curve",)),
    "link": (_on("track_link_fresh"), _off("track_link_fresh"), ("link_fresh", "link_hist")),
    "delay": (_on("track_delay"), _off("track_delay"), ("delay_sum", "delay_max", "delay_bins")),
    "delay_dist": (_on("track_delay_dist"), _off("track_delay_dist"), ("delay_dist", "delay_dist_bins")),
    "watch": (lambda e: e.watch(WATCHED), lambda e: e.watch([]), ("watch_first", "watch_arrival", "watch_ptr")),
}
NAMES = list(RECORDS)
ARC_WALKERS = ("load", "fresh", "fresh_curve", "link", "mult", "watch")   # what lossy and delayed links refuse
CALLS = {"load": "gp_track_load", "fresh": "gp_track_fresh", "fresh_curve": "gp_track_fresh_curve",
         "link": "gp_track_link_fresh", "mult": "gp_track_mult", "watch": "gp_watch"}   # the refusal names the call to undo
PARTITION_KEEPS = ("curve", "delay", "delay_dist")                          # kept for the owned slice
SHAPES = {"w2": (70, 2, 2), "w1": (40, 1, 1)}                               # messages, inject rounds, W
CASES = [(name, "w2") for name in NAMES] + [("delay", "w1"), ("delay_dist", "w1")]
CASE_IDS = [f"{name}-{shape}" for name, shape in CASES]


@functools.lru_cache(maxsize=None)
def _shape(shape):
    import _gossip_pkg
    pkg = _gossip_pkg.load()
    m, rounds, _ = SHAPES[shape]
    g = pkg.overlay.barabasi_albert(N, BA_M, SEED)
    origin = pkg.overlay.random_origins(g.n, m, seed=SEED)
    inject = (np.arange(m) % rounds).astype(np.int32)
    return g, origin, inject


def engine(pkg, shape, names=(), **cfg):
    """an engine on the shape with the records `names` asked for, not reset yet"""
    g, origin, inject = _shape(shape)
    eng = pkg.GossipEngine(0, **cfg)
    eng.load_graph(g)
    eng.set_messages(origin, inject)
    assert eng.info()[3] == SHAPES[shape][2]
    for name in names:
        RECORDS[name][0](eng)
    return eng


def reads(eng, name):
    return {r: getattr(eng, r)().copy() for r in RECORDS[name][2]}


def status(pkg, fn):
    with pytest.raises(pkg.GossipError) as e:
        fn()
    return e.value.status


def all_refused(pkg, eng, name, code):
    for r in RECORDS[name][2]:
        assert status(pkg, getattr(eng, r)) == code, (name, r)


def same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


_ALL = {}


def all_on(pkg, shape):
    """every record's reads, from one run that keeps all nine: at the end of
    the run and as they stand after round 2; computed once per shape"""
    if shape not in _ALL:
        inject = _shape(shape)[2]
        with engine(pkg, shape, NAMES) as eng:
            eng.reset()
            stats = [eng.round(), eng.round()]
            at2 = {name: reads(eng, name) for name in NAMES}
            while not (stats[-1]["new_bits"] == 0 and stats[-1]["round"] >= int(inject.max())):
                stats.append(eng.round())
            end = {name: reads(eng, name) for name in NAMES}
            for r in ("fresh_recv", "sole_recv", "delay_sum", "link_fresh", "load_recv"):   # the run says something
                assert any(r in v and v[r].any() for v in end.values()), r
            assert (end["watch"]["watch_first"] != 255).any()
        assert len(stats) > 3
        _ALL[shape] = {"rounds": len(stats), "at2": at2, "end": end}
    return _ALL[shape]


def finish(eng, shape, done):
    inject = _shape(shape)[2]
    st = None
    for _ in range(done, 254):
        st = eng.round()
        if st["new_bits"] == 0 and st["round"] >= int(inject.max()):
            break
    return st["round"] + 1


@pytest.mark.parametrize("name,shape", CASES, ids=CASE_IDS)
def test_lifecycle(pkg, monkeypatch, name, shape):
    monkeypatch.delenv("GP_LOAD_EAGER", raising=False)
    lib = pkg._lib
    want = all_on(pkg, shape)
    with engine(pkg, shape) as eng:
        all_refused(pkg, eng, name, lib.GP_ENOTRACK)                  # no run state, nothing asked for
        eng.reset()
        all_refused(pkg, eng, name, lib.GP_ENOTRACK)                  # not tracked
        RECORDS[name][0](eng)
        all_refused(pkg, eng, name, lib.GP_ENOTRACK)                  # takes effect at the next reset
        eng.reset()
        blob0 = eng.checkpoint()
        eng.round(), eng.round()
        same(reads(eng, name), want["at2"][name])
        blob2 = eng.checkpoint()
        assert finish(eng, shape, 2) == want["rounds"]
        same(reads(eng, name), want["end"][name])
        eng.restore(blob2)                                            # past round 0: the record is not in the blob
        if name == "load":                                            # (a lazy run's totals are a function of its state)
            same(reads(eng, name), want["at2"][name])
        else:
            all_refused(pkg, eng, name, lib.GP_ESTATE)
        eng.reset()                                                   # a reset makes the reads succeed again
        fresh_run = reads(eng, name)
        eng.restore(blob0)                                            # at round 0: nothing counted yet, still valid
        same(reads(eng, name), fresh_run)
        assert finish(eng, shape, 0) == want["rounds"]
        same(reads(eng, name), want["end"][name])
        RECORDS[name][1](eng)                                         # off: still read until the next reset
        same(reads(eng, name), want["end"][name])
        eng.reset()
        all_refused(pkg, eng, name, lib.GP_ENOTRACK)
        # a second record beside it: the reset reallocates, both read right
        other = NAMES[(NAMES.index(name) + 1) % len(NAMES)]
        RECORDS[name][0](eng)
        eng.reset()
        RECORDS[other][0](eng)
        all_refused(pkg, eng, other, lib.GP_ENOTRACK)
        eng.reset()
        assert finish(eng, shape, 0) == want["rounds"]
        same(reads(eng, name), want["end"][name])
        same(reads(eng, other), want["end"][other])


def test_eager_load_is_lost_by_a_restore(pkg, monkeypatch):
    """GP_LOAD_EAGER=1 (read at gp_create): the per-round totals are not in the blob"""
    monkeypatch.setenv("GP_LOAD_EAGER", "1")
    lib = pkg._lib
    want = all_on(pkg, "w2")   # (itself eager here or lazy, whichever ran first: the totals are the same)
    with engine(pkg, "w2", ["load"]) as eng:
        eng.reset()
        blob0 = eng.checkpoint()
        eng.round(), eng.round()
        same(reads(eng, "load"), want["at2"]["load"])
        blob2 = eng.checkpoint()
        eng.restore(blob2)
        all_refused(pkg, eng, "load", lib.GP_ESTATE)
        eng.restore(blob0)
        assert finish(eng, "w2", 0) == want["rounds"]
        same(reads(eng, "load"), want["end"]["load"])


def test_a_crash_makes_a_lazy_load_eager(pkg, monkeypatch):
    """an explicit crash turns liveness on: from there the run counts per round
    and a restore past round 0 loses the totals"""
    monkeypatch.delenv("GP_LOAD_EAGER", raising=False)
    lib = pkg._lib
    with engine(pkg, "w2", ["load"]) as eng:
        eng.reset()
        eng.round()
        eng.crash([5])
        eng.round()
        blob2 = eng.checkpoint()
        eng.round()
        eng.load_sent()
        eng.restore(blob2)
        all_refused(pkg, eng, "load", lib.GP_ESTATE)
        eng.reset()
        assert not eng.load_sent().any()


@pytest.mark.parametrize("link", ["loss", "delay"])
@pytest.mark.parametrize("name", NAMES)
def test_lossy_and_delayed_links_refuse_the_arc_walkers(pkg, name, link):
    lib = pkg._lib
    with engine(pkg, "w2", [name]) as eng:
        eng.reset()
        if link == "loss":
            eng.link_loss(0.1, seed=3)
        else:
            eng.link_delay(2, seed=3)
        if name in ARC_WALKERS:
            with pytest.raises(pkg.GossipError) as e:
                eng.reset()
            assert e.value.status == lib.GP_EINVAL
            assert CALLS[name] in str(e.value) and ("link loss" if link == "loss" else "link delay") in str(e.value)
            RECORDS[name][1](eng)                                     # without the record the links are taken
            eng.reset()
            all_refused(pkg, eng, name, lib.GP_ENOTRACK)
        else:
            eng.reset()
            run(eng, _shape("w2")[2])
            for r in RECORDS[name][2]:
                getattr(eng, r)()
        assert (eng.link_loss_info()[0], eng.link_delay_info()[0]) == (link == "loss", link == "delay")


def test_two_partition_contexts(pkg):
    """through round_group: the six single-rank records are refused, the spread
    curve, the receipt delays and their distributions are kept for the owned slice"""
    lib = pkg._lib
    want = all_on(pkg, "w2")
    engs = []
    try:
        for k in range(2):
            e = engine(pkg, "w2")
            e.set_partition(k, 2)
            e.set_messages(*_shape("w2")[1:])
            for name in NAMES:
                RECORDS[name][0](e)
            e.reset()
            engs.append(e)
        stats = pkg.GossipEngine.run_group(engs)
        assert len(stats) == want["rounds"]
        for name in NAMES:
            if name not in PARTITION_KEEPS:
                for e in engs:
                    all_refused(pkg, e, name, lib.GP_ENOTRACK)
        lo = 0
        curve = 0
        for e in engs:
            vb, ve = e.partition()
            assert vb == lo and ve > vb
            lo = ve
            assert np.array_equal(e.delay_sum(), want["end"]["delay"]["delay_sum"][vb:ve])
            assert np.array_equal(e.delay_max(), want["end"]["delay"]["delay_max"][vb:ve])
            assert np.array_equal(e.delay_dist(), want["end"]["delay_dist"]["delay_dist"][vb:ve])
            assert e.delay_sum().shape == (ve - vb,) and e.delay_dist().shape == (ve - vb, 16)
            curve = curve + e.curve().astype(np.int64)
        assert lo == N
        assert np.array_equal(curve, want["end"]["curve"]["curve"].astype(np.int64))
    finally:
        for e in engs:
            e.close()
