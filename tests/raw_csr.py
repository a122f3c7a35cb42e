"""An in-CSR with self-loops, repeated arcs and unsorted in-lists, loaded as
given (gp_load_graph): the overlay of
test_gpu_parity.py::test_raw_csr_self_loops_and_repeated_arcs, shared with
test_gpu_records_matrix.py.  A self-loop or a repeated arc is one more link of
the sends (deg) and of the per-arc records, and can never bring a vertex
anything it does not hold.
"""
import functools

import numpy as np


def _csr(n, s, d):
    """in-CSR of the arcs s[i] -> d[i], every in-list in the order given"""
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, d + 1, 1)
    rp = np.cumsum(rp)
    col = np.empty(s.size, np.int32)
    cur = rp[:-1].copy()
    for u, v in zip(s.tolist(), d.tolist()):
        col[cur[v]] = u
        cur[v] += 1
    return rp, col


@functools.lru_cache(maxsize=None)
def _arrays():
    import _gossip_pkg
    pkg = _gossip_pkg.load()
    g0 = pkg.overlay.barabasi_albert(3000, 3, seed=41)
    rng = np.random.default_rng(41)
    src, dst = g0.arcs()
    loops = rng.choice(g0.n, 300, replace=False)
    again = rng.choice(src.size, 2000, replace=False)   # repeated arcs, both directions
    s = np.concatenate([src, loops, src[again], dst[again]])
    d = np.concatenate([dst, loops, dst[again], src[again]])
    order = rng.permutation(s.size)   # in-lists in no particular order
    s, d = s[order], d[order]
    return (g0.n,) + _csr(g0.n, s, d)


def loops_and_repeats(pkg):
    """Barabasi-Albert(3000, 3) with 300 self-loops and 2000 arcs repeated in
    both directions, the in-lists permuted"""
    n, rp, col = _arrays()
    return pkg.CSR(n, rp.copy(), col.copy(), False)


def simple_copy(pkg, g):
    """g without its self-loops, every repeated arc once (in-lists sorted)"""
    rp = np.asarray(g.row_ptr, np.int64)
    src = np.asarray(g.col, np.int64)
    dst = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(rp))
    pairs = np.unique(np.stack([dst, src], axis=1)[src != dst], axis=0)
    rp2, col2 = _csr(int(g.n), pairs[:, 1], pairs[:, 0])
    return pkg.CSR(int(g.n), rp2, col2, False)
