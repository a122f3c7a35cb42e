"""Three tiny overlays with a long diameter, and their message tables: the
shapes of test_long_runs_ref.py and test_gpu_long_runs.py, whose floods are
still under way when the engine's 254-round ceiling cuts them.

Every overlay is a raw symmetric in-CSR (raw_csr._csr):

  path(pkg, 300)     0 - 1 - ... - 299.  A message injected at vertex 0 in round
                     0 reaches vertex v in round v, v <= 254; vertices 255 .. 299
                     never hear it (first = 255 beside 254).
  far_hubs(pkg)      path(300) with 100 leaves on vertex 130 (ids 300 .. 399)
                     and 100 on vertex 250 (ids 400 .. 499): n = 500, both
                     centres of in-degree 102, hubs at hub_threshold = 64.
  thick_ring(pkg)    the circulant v ~ v +- 1, v +- 2 on 1100 vertices: a flood
                     advances two vertices per round in both directions
                     (diameter 275) and survives isolated crashes and closed arcs.

Tables (table(pkg, g, kind, m)), STEP = the vertices a flood advances per round:

  "ends"     origins alternate between vertex 0 and vertex 299 (on the ring:
             random_origins), inject rounds k % 3.
  "late"     "ends" with its last 32 messages injected late, in two groups.
             LATE: rounds 100, 200, every round of 240 .. 253, and 253 twice
             more (18 messages), at vertices 0, 299, 150 and 5 in turn; the
             round-253 messages sit at 5, 0 and 299: an injection of round 253
             gives first = 253 at its origin and 254 at the neighbours.
             The FAN: inject rounds 240 .. 253 at the vertices
             FAN_AT - STEP * (254 - round), which all reach vertex FAN_AT in
             receipt round 254 with the delays 14 .. 1: delay_dist's window
             lists 14 present inject rounds there, and FAN_AT holds every
             column 1 .. 14 beside the saturated one.  (A delay is the distance
             to the origin, so the four vertices of LATE alone give a vertex
             at most four distinct delays.)
  "uniform"  every message at vertex 0 in round 0.
  "leaves"   far_hubs only: origin[k] = 300 + k % 200, inject[k] = 128 +
             (k // 2) % 120.  Every message starts late at a leaf of one of
             the two hubs, so that under loss and repair (repair_long_cases.py)
             the leaves hold what their hub still misses and the hubs get
             non-empty offers in the rounds past 128.
"""
import functools

import numpy as np

import raw_csr

CEILING = 254          # rounds the engine runs at most; the largest receipt round
FAN_AT = 150
LATE_ROUNDS = [100, 200] + list(range(240, 254)) + [253, 253]
LATE_VERTS = (0, 299, 150, 5)
WORDS = {100: 2, 200: 4, 1000: 16, 4096: 64}


def _sym(pkg, n, a, b):
    """the undirected overlay of the edges a[i] - b[i]"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    rp, col = raw_csr._csr(n, np.concatenate([a, b]), np.concatenate([b, a]))
    return pkg.CSR(n, rp, col, False)


@functools.lru_cache(maxsize=None)
def _path_edges(n):
    a = np.arange(n - 1, dtype=np.int64)
    return a, a + 1


def path(pkg, n=300):
    return _sym(pkg, n, *_path_edges(n))


def far_hubs(pkg):
    a, b = _path_edges(300)
    a = np.concatenate([a, np.full(100, 130), np.full(100, 250)])
    b = np.concatenate([b, np.arange(300, 400), np.arange(400, 500)])
    g = _sym(pkg, 500, a, b)
    deg = np.diff(np.asarray(g.row_ptr, np.int64))
    assert g.n == 500 and deg[130] == 102 and deg[250] == 102 and np.sort(deg)[-3] == 2
    return g


def thick_ring(pkg, n=1100):
    v = np.arange(n, dtype=np.int64)
    return _sym(pkg, n, np.concatenate([v, v]), np.concatenate([(v + 1) % n, (v + 2) % n]))


def step_of(g):
    """vertices a flood advances per round: 2 on the ring, 1 on the path shapes"""
    return 2 if int(np.diff(np.asarray(g.row_ptr, np.int64)).min()) == 4 else 1


def late_tail(step):
    """(origin, inject) of the 32 late messages: LATE, then the FAN"""
    origin = [LATE_VERTS[i % 4] for i in range(len(LATE_ROUNDS))]
    inject = list(LATE_ROUNDS)
    for r in range(240, 254):
        origin.append(FAN_AT - step * (CEILING - r))
        inject.append(r)
    return np.array(origin, np.int32), np.array(inject, np.int32)


def table(pkg, g, kind, m):
    """(origin, inject) int32 [m] of table `kind` on overlay g"""
    if kind == "uniform":
        return np.zeros(m, np.int32), np.zeros(m, np.int32)
    if kind == "leaves":
        if g.n != 500:
            raise ValueError("the leaves table is far_hubs's")
        k = np.arange(m)
        return (300 + k % 200).astype(np.int32), (128 + (k // 2) % 120).astype(np.int32)
    if step_of(g) == 2:
        origin = np.asarray(pkg.overlay.random_origins(g.n, m, seed=m), np.int32).copy()
    else:
        origin = np.where(np.arange(m) % 2 == 0, 0, 299).astype(np.int32)
    inject = (np.arange(m) % 3).astype(np.int32)
    if kind == "late":
        o, i = late_tail(step_of(g))
        origin[m - o.size:], inject[m - i.size:] = o, i
    elif kind != "ends":
        raise ValueError(kind)
    return origin, inject


def late_counts(first):
    """what a run holds at and past the middle of the u8 range: (cells with
    128 <= first <= 254, cells with first == 254, cells never reached)"""
    return int(((first >= 128) & (first != 255)).sum()), int((first == 254).sum()), int((first == 255).sum())
