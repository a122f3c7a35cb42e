"""The references at the 254-round ceiling, pinned on the CPU before
test_gpu_long_runs.py compares the engine with them (shapes: long_shapes.py).

A receipt round is a u8 with 255 = never, so a run of 254 rounds holds the
value 254 right beside the sentinel; the C oracle, the per-peer sha256 harness
and the record references (delay_ref, delay_dist_ref, link_ref, mult_ref,
lossy_ref) must agree there and give the closed forms of a path.
"""
import numpy as np
import pytest

import delay_dist_ref
import delay_ref
import link_ref
import long_shapes as ls
import lossy_ref
import mult_ref
from test_oracle import _both

# a 12-message table in the style of "late": vertex 0 is the origin of a round-253 message
LATE12 = (np.array([0, 299, 0, 299, 150, 5, 0, 299, 150, 0, 299, 5], np.int32),
          np.array([0, 1, 2, 0, 100, 200, 240, 250, 252, 253, 253, 253], np.int32))
CRASHES = [(200, 199), (40, 250), (0, 253), (120, 100)]


@pytest.mark.parametrize("kw", [dict(), dict(crashes=CRASHES), dict(churn=True, p_fail=0.0005, churn_seed=3)],
                         ids=["plain", "crashes", "churn"])
def test_oracle_equals_harness_at_the_ceiling(pkg, oracle, harness, kw):
    g = ls.far_hubs(pkg)
    origin, inject = LATE12
    ref = _both(pkg, oracle, harness, g, origin, inject, **kw)
    first = ref["first"]
    assert ref["rounds"] == 254
    assert int(first[first != 255].max()) == 254
    late, last, never = ls.late_counts(first)
    print(f"{kw}: {late} cells with first >= 128, {last} with 254, {never} never, "
          f"{sum(s['crashed'] for s in ref['stats'][128:])} crashes and "
          f"{sum(s['removals'] for s in ref['stats'][128:])} removals in rounds >= 128")
    if "crashes" in kw:   # the origin of a round-253 message crashes in round 253: the message is lost
        assert ref["stats"][253]["lost"] == 1 and ref["stats"][253]["injected"] == 2
        assert (first[:, 9] == 255).all()
    if not kw:
        assert first[254, 0] == 254 and first[255, 0] == 255


@pytest.fixture(scope="module")
def path_run(pkg, oracle):
    g = ls.path(pkg)
    m = 100
    origin, inject = ls.table(pkg, g, "uniform", m)
    return g, m, inject, oracle.run(g, origin, inject, want_first=True)


def test_path_first_receipts(pkg, path_run):
    g, m, inject, ref = path_run
    first = ref["first"]
    assert ref["rounds"] == 254
    for v in range(300):
        assert (first[v] == (v if v <= 254 else 255)).all(), v
    d = delay_ref.totals(ref, inject)
    assert int(d["max"].max()) == 254 and d["max"].tolist() == [v if v <= 254 else 0 for v in range(300)]
    assert d["sum"].tolist() == [m * v if v <= 254 else 0 for v in range(300)]
    dist = delay_dist_ref.totals(ref, inject)["dist"]
    for v in range(300):
        want = np.zeros(16, np.int64)
        if v <= 254:
            want[min(v, 15)] = m
        assert np.array_equal(dist[v], want), v
    hist = np.stack([(first == r).sum(axis=0) for r in range(255)])
    assert hist.shape == (255, m) and (hist == 1).all()   # one vertex per row, rows 0 .. 254


def test_path_closed_form_records(pkg, path_run):
    g, m, inject, ref = path_run
    rec = link_ref.record(g, ref)
    src, dst, link = rec["src"], rec["dst"], rec["link"]
    fwd = (dst == src + 1) & (dst <= 254)
    assert int(fwd.sum()) == 254 and (link[fwd] == m).all() and not link[~fwd].any()
    assert len(rec["per_round"]) == 254 and int(rec["per_round"][252].sum()) == 253 * m
    mult = mult_ref.totals(g, ref)
    assert int(mult["hist"][1]) == 254 * m and int(mult["hist"][0]) == m and not mult["hist"][2:].any()
    assert mult["sole_recv"].tolist() == [m if 1 <= v <= 254 else 0 for v in range(300)]
    assert mult["sole_sent"].tolist() == [m if v <= 253 else 0 for v in range(300)]


def test_lossy_ref_with_open_arcs_is_the_oracles_run(pkg, oracle):
    g = ls.thick_ring(pkg)
    origin, inject = ls.table(pkg, g, "ends", 100)
    ref = oracle.run(g, origin, inject, want_first=True)
    got = lossy_ref.run(g, origin, inject, p=0.0, seed=11)
    assert ref["rounds"] == 254 and got["rounds"] == 254
    late, last, never = ls.late_counts(ref["first"])
    print(f"thick_ring x ends: {late} cells with first >= 128, {last} with 254, {never} never reached")
    assert late >= 10_000 and last > 0 and never > 0
    assert np.array_equal(got["first"], ref["first"])
    for a, b in zip(got["stats"], ref["stats"]):
        for k in ("injected", "new_bits", "receivers", "sends", "active"):
            assert a[k] == b[k], (k, a["round"], a[k], b[k])
    assert np.array_equal(got["coverage"], ref["coverage"])
    assert np.array_equal(got["forwards"], ref["forwards"])
