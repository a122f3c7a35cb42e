"""Child process of tests/test_gpu_delay_dist.py (TEST INFRASTRUCTURE).

Loads the engine built against the in-process RCCL stand-in (GOSSIP_HIP_LIB =
_build/libgossip_hip_rccl_standin.so, tests/native/rccl_standin.cpp) and runs a
vertex partition of P = 2 ranks as two threads on one GPU with
gp_track_delay_dist on: every round goes through exchange_rccl, and each rank
keeps the delay distributions of its owned vertices.  The owned slices must
concatenate to tests/delay_dist_ref.py's array of the oracle's one-context run,
the tables add up to the whole overlay's -- once with a table of several inject
rounds (the row pass over the owned frontier rows) and once with one inject
round (the guard-word pass).

Prints "delay_dist cases ok: N" and exits 0 when every case matches.
"""
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _gossip_pkg  # noqa: E402
import delay_dist_ref  # noqa: E402
from oracle import lib as oracle  # noqa: E402

P = 2


def run_ranks(pkg, g, origin, inject):
    uid = pkg.GossipEngine.comm_unique_id()
    engs = []
    for k in range(P):
        e = pkg.GossipEngine(0)
        e.load_graph(g)
        e.set_partition(k, P)
        e.set_messages(origin, inject)
        e.track_delay_dist()
        e.reset()
        engs.append(e)
    last = int(np.max(inject))
    out, errs = [None] * P, []

    def rank(k):
        try:
            e = engs[k]
            e.comm_init(uid, P, k)
            stats = []
            for r in range(254):
                stats.append(e.round())
                if stats[-1]["new_bits"] == 0 and r >= last:
                    break
            out[k] = dict(stats=stats, dist=e.delay_dist(), seenpop=e.seenpop(), bins=e.delay_dist_bins(),
                          part=e.partition())
        except BaseException as exc:   # surfaced below, after every thread ended
            errs.append((k, exc))

    ts = [threading.Thread(target=rank, args=(k,)) for k in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for e in engs:
        e.close()
    if errs:
        raise RuntimeError(f"rank failures: {[(k, repr(e)) for k, e in errs]}")
    return out


def main():
    pkg = _gossip_pkg.load()
    assert "standin" in os.environ.get("GOSSIP_HIP_LIB", ""), "set GOSSIP_HIP_LIB to the stand-in build"
    g = pkg.overlay.barabasi_albert(3001, 2, seed=8)
    origin = pkg.overlay.random_origins(g.n, 200, seed=8)
    cases = 0
    for inject in ((np.arange(200) % 4).astype(np.int32), np.zeros(200, np.int32)):
        ref = oracle.run(g, origin, inject, want_first=True)
        exp = delay_dist_ref.totals(ref, inject)
        out = run_ranks(pkg, g, origin, inject)
        assert [o["part"] for o in out] == pkg.dist.partition_bounds(g.n, P, None)
        assert all(len(o["stats"]) == ref["rounds"] for o in out)
        assert sum(s["xchg_rows"] for s in out[0]["stats"]) > 0
        for o in out:
            lo, hi = o["part"]
            assert o["dist"].shape == (hi - lo, 16) and o["dist"].dtype == np.uint16
            assert np.array_equal(o["bins"], delay_dist_ref.bins(g, exp["dist"], lo=lo, hi=hi))
        assert np.array_equal(np.concatenate([o["dist"] for o in out]).astype(np.int64), exp["dist"])
        assert np.array_equal(np.concatenate([o["seenpop"] for o in out]).astype(np.int64), exp["seenpop"])
        assert np.array_equal(pkg.latency.dist_combine([o["bins"] for o in out]),
                              delay_dist_ref.bins(g, exp["dist"]).astype(np.int64))
        cases += 1
    print(f"delay_dist cases ok: {cases}", flush=True)


if __name__ == "__main__":
    main()
