"""bench.py host logic (no GPU): the committed PMC traffic measurements are
picked by workload, and never for a run of another shape."""
import glob
import json
import os

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pmc_traffic_matches_its_own_workload():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "pmc_traffic*.json")))
    assert files, "no PMC traffic measurement committed under profiles/"
    for path in files:
        d = json.load(open(path))
        traffic, src = bench.pmc_traffic(d["config"])
        assert src == os.path.relpath(path, ROOT)
        assert traffic == d["traffic_bytes_per_launch"]
        assert d["traffic_bytes_per_launch"] >= 0.5 * d["alg_bytes_per_launch"]


def test_pmc_traffic_none_for_other_shape():
    d = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    cfg = dict(d["config"], messages=d["config"]["messages"] // 2)
    assert bench.pmc_traffic(cfg) == (None, None)


def test_pmc_traffic_none_for_other_message_order():
    """A measurement taken with one message order is not used for a run of the other."""
    d = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    cfg = dict(d["config"], message_order="given")
    assert d["config"]["message_order"] != "given"
    assert bench.pmc_traffic(cfg) == (None, None)


def test_plain_run_is_the_default():
    """The CPU baseline legs and the degree check run only under --full."""
    assert bench.parse([]).full is False and bench.parse([]).dump_outputs is None
    assert bench.parse(["--full"]).full is True


def test_dump_outputs_exact_and_bounded(tmp_path):
    """--dump-outputs: float64 files that hold the step's integers exactly; the
    digest as 32-bit halves of all vertices, or of a fixed sample of them."""
    rng = np.random.default_rng(1)
    stats = [dict.fromkeys(bench.DUMP_STATS, 0) | {"new_bits": 47881074578, "sends": r} for r in range(3)]
    cov = rng.integers(0, 1 << 26, 130, dtype=np.uint64)
    fwd = rng.integers(0, 1 << 40, 130, dtype=np.uint64)
    for n in (1000, bench.DUMP_MAX_VERTICES + 77):
        dig = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        out = tmp_path / str(n)
        bench.dump_outputs(str(out), stats, (dig, cov, fwd))
        got = {p.stem: np.load(p) for p in out.iterdir()}
        assert all(a.dtype == np.float64 for a in got.values())
        assert sum(a.nbytes for a in got.values()) <= 64 << 20
        assert got["round_stats"].shape == (3, len(bench.DUMP_STATS))
        assert got["round_stats"][:, bench.DUMP_STATS.index("new_bits")].tolist() == [47881074578] * 3
        assert np.array_equal(got["coverage"].astype(np.uint64), cov)
        assert np.array_equal(got["forwards"].astype(np.uint64), fwd)
        v = got["digest_vertices"].astype(np.int64)
        assert len(v) == min(n, bench.DUMP_MAX_VERTICES) and np.all(np.diff(v) > 0) and v[-1] < n
        d = got["digest"].astype(np.uint64)
        assert np.array_equal((d[:, 0] << np.uint64(32)) | d[:, 1], dig[v])
        again = tmp_path / f"{n}_again"   # the sample is fixed: a second dump lists the same vertices
        bench.dump_outputs(str(again), stats, (dig, cov, None))
        assert np.array_equal(np.load(again / "digest_vertices.npy"), got["digest_vertices"])
        assert not (again / "forwards.npy").exists()
    part = tmp_path / "part"   # vertex partition: the counters only
    bench.dump_outputs(str(part), stats, None)
    assert [p.name for p in part.iterdir()] == ["round_stats.npy"]


def test_round_bytes_terms():
    """Algorithmic bytes of a pull launch: per-vertex state,
    arcs by scan mode, row bytes, seen rows, written rows with their committed
    words, and the senders' rows k_mklm reads."""
    n, W = 1000, 64
    base = dict(arcs_scanned=0, row_bytes=0, seen_rows_read=0, rows_written=0, scan=0)
    assert bench.round_bytes(base, W, n) == 30 * n
    assert bench.round_bytes(dict(base, arcs_scanned=10), W, n) == 30 * n + 120
    assert bench.round_bytes(dict(base, arcs_scanned=10, scan=2), W, n) == 30 * n + 40
    assert bench.round_bytes(dict(base, row_bytes=777), W, n) == 30 * n + 777
    assert bench.round_bytes(dict(base, seen_rows_read=3), W, n) == 30 * n + 3 * 512
    assert bench.round_bytes(dict(base, rows_written=2), W, n) == 30 * n + 2 * (512 + 23)
    assert bench.round_bytes(dict(base, lm_rows=5), W, n) == 30 * n + 5 * 512
