"""The lossy repair cases tests/test_repair_ref.py (the conditions, on the
reference alone) and tests/test_gpu_repair.py (the engine) share, computed once
per process: test_gpu_link_loss.py's overlay and tables at p = 0.5, loss seed
11, repair seed 21, stepped for at most CUT rounds."""
import functools

import lossy_ref
import repair_ref

P, SEED, RSEED, CUT = 0.5, 11, 21, 48
PERIODS = (1, 3)
MIN_SHARE = 0.15   # of the first-receipt cells repair must change against the lossy run without it (m >= 64)


@functools.lru_cache(maxsize=None)
def table(n, m):
    from test_gpu_curve import _width_ref
    return _width_ref(n, m)   # g, origin, inject, the C oracle's flood


@functools.lru_cache(maxsize=None)
def plain(n, m, p=P, seed=SEED):
    g, origin, inject, _ = table(n, m)
    return lossy_ref.run(g, origin, inject, p=p, seed=seed)


@functools.lru_cache(maxsize=None)
def repaired(n, m, period, p=P, seed=SEED, rseed=RSEED, max_rounds=CUT):
    g, origin, inject, _ = table(n, m)
    return repair_ref.run(g, origin, inject, p=p, seed=seed, period=period, rseed=rseed, max_rounds=max_rounds)


def changed_share(a, b):
    return float((a["first"] != b["first"]).mean())
