"""Shape and runs of tests/test_gpu_lane_ops.py, and its child process.

The commit-path shape: one flood to quiescence on a Chung-Lu overlay of 4,096
peers (mean degree 8, gamma 2.5) with m messages in spread order, every round
a pull, the packed gather and the per-line rule forced on.  As a program it
runs the W = 64 case with the library GOSSIP_HIP_LIB names -- the GP_LANE_OPS=0
test build -- and saves every output and counter for the parent to compare:

    python lane_ops_driver.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DBAR, GAMMA = 4096, 8, 2.5
HUB_THRESHOLD = 64
WIDTHS = {64: 4096, 32: 2048, 16: 1024, 8: 512}   # W: messages
OUTPUTS = ("seen", "digest", "coverage", "forwards")
# counters of the hub chunks' early-exit rounds that depend on wave timing (csrc/hub.hip)
TIMING_KEYS = ("arcs_scanned", "rows_gathered", "row_bytes")
TIME_KEYS = ("expand_ms", "exchange_ms", "round_ms", "kernel_ms")


def overlay(pkg, oracle):
    rp, col = oracle.chung_lu(N, DBAR, GAMMA, 5)
    return pkg.CSR(N, rp, col, False)


def messages(pkg, g, m):
    """m messages in spread order, as the bench runs them."""
    origin = pkg.overlay.random_origins(g.n, m, seed=5)
    return origin[pkg.overlay.spread_order(pkg.overlay.spread_keys(g.row_ptr, g.col, origin, 3), None)]


def run(pkg, g, origin, hub_threshold):
    """One run to quiescence (GP_LINE_PACK / GP_LINE_DONE are read at gp_create:
    the caller has set them)."""
    cfg = dict(track_first=0, track_digest=1, push_ratio=0.0, unfiltered_pct=1, hub_threshold=hub_threshold)
    with pkg.GossipEngine(0, **cfg) as eng:
        eng.load_graph(g)
        eng.set_messages(origin, None)
        eng.reset()
        stats = eng.run()
        eng.finalize()
        return dict(stats=stats, seen=eng.seen(), digest=eng.digest(), coverage=eng.coverage(), forwards=eng.forwards())


def counters(stats, drop=()):
    """The rounds' counters as one integer matrix (no timings)."""
    keys = [k for k in sorted(stats[0]) if k not in TIME_KEYS and k not in drop]
    return keys, np.array([[int(s[k]) for k in keys] for s in stats], dtype=np.uint64)


def set_env(env):
    env["GP_LINE_PACK"] = "1"
    env["GP_LINE_DONE"] = "1"
    env["GP_LINE_DONE_MIN_DEG"] = "16"


def main(out):
    sys.path.insert(0, ROOT)
    import _gossip_pkg
    from oracle import lib as oracle
    set_env(os.environ)
    oracle.load()
    pkg = _gossip_pkg.load()
    g = overlay(pkg, oracle)
    origin = messages(pkg, g, WIDTHS[64])
    save = {}
    for tag, thr in (("hub", HUB_THRESHOLD), ("flat", int(np.diff(g.row_ptr).max()) + 1)):
        r = run(pkg, g, origin, thr)
        for k in OUTPUTS:
            save[f"{tag}_{k}"] = r[k]
        keys, mat = counters(r["stats"])
        save[f"{tag}_counters"] = mat
        save[f"{tag}_keys"] = np.array(keys)
    save["lib"] = np.array(pkg._lib.load()._name)
    np.savez(out, **save)
    print("lane-off runs ok:", save["lib"])


if __name__ == "__main__":
    main(sys.argv[1])
