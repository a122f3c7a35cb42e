"""In-register lane operations of the pull family (csrc/lane_ops.h, DESIGN.md
§3.3): DPP row operations, v_permlane16/32_swap and v_readlane in place of the
`__shfl_xor` butterflies (ds_bpermute_b32).

Sums, xors and ORs of integers are order-free, so every output and every
counter must stay bit for bit what the LDS form computes -- the reference's
Message-List dedup (Peer.py:175-216) and its send loop over every link
(Peer.py:402-404), whose new bits the sums count and whose digest the xors fold.

 - the primitives, through gp_selftest_lane_ops: every operation against its
   `__shfl_xor` form in the same kernel, and against numpy here;
 - the commit path at every row width the pull family is built for (W = 64,
   32, 16, 8) against the C oracle, on a shape that takes the serial loop, the
   packed gather, the done-neighbour pairs / quads / groups, gather_pairs and
   the hub kernels (tests/lane_ops_driver.py);
 - the W = 64 case against the same run of the GP_LANE_OPS=0 test build
   (build_lib.build_lane_off) in a child process.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import lane_ops_driver as drv
from test_gpu_line_done import STAT_KEYS, _check_oracle, _work

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED1A2E
WAVES, PATTERNS = 4, 68
U64 = np.uint64


def _mix(z):
    z = z + U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def _values(seed):
    """[pattern][wave][lane]: ls_value of csrc/lane_selftest.hip."""
    x = np.zeros((PATTERNS, WAVES, 64), dtype=U64)
    w = np.arange(WAVES, dtype=U64)[:, None]
    l = np.arange(64, dtype=U64)[None, :]
    x[1] = ~U64(0)
    one = _mix(np.full((WAVES, 1), seed, dtype=U64) ^ (w + U64(1))) | U64(1)
    for k in range(64):
        x[2 + k, :, k] = one[:, 0]
    x[66] = np.broadcast_to(l * U64(0x0000000100000001), (WAVES, 64))
    x[67] = _mix(np.full((WAVES, 64), seed, dtype=U64) ^ ((w * U64(64) + l + U64(1)) * U64(0xD1B54A32D192ED03)))
    return x


def _group(x, n, op):
    """Reduction over aligned groups of n lanes, every lane holding its group's."""
    g = op.reduce(x.reshape(x.shape[:-1] + (64 // n, n)), axis=-1, keepdims=True, dtype=x.dtype)   # (wraps at the type's width)
    return np.broadcast_to(g, x.shape[:-1] + (64 // n, n)).reshape(x.shape)


def _slots(x, lpr):
    """OR over the lanes lpr, 2 lpr, .. apart: every lane its residue class's."""
    g = np.bitwise_or.reduce(x.reshape(x.shape[:-1] + (64 // lpr, lpr)), axis=-2, keepdims=True)
    return np.broadcast_to(g, x.shape[:-1] + (64 // lpr, lpr)).reshape(x.shape)


def _expected_sums(seed):
    x = _values(seed)
    kinds = ((x.astype(np.uint32), np.add), (x, np.add), (x, np.bitwise_xor), (x, np.bitwise_or),
             ((x & U64(1)).astype(np.uint32), np.bitwise_or))
    out = []
    with np.errstate(over="ignore"):
        for v, op in kinds:
            for n in (4, 8, 16, 32, 64):
                out.append(int(_group(v, n, op).astype(U64).sum(dtype=U64)))
        for lpr in (32, 16, 8, 4, 32, 16, 8):   # the row widths, then the packed layouts
            out.append(int(_slots(x, lpr).sum(dtype=U64)))
    return out


def test_primitives(pkg):
    """Every operation and group size: 4 waves of all zero, all ones, each
    single lane, the lane index and seeded random words; no lane differs from
    the `__shfl_xor` form, and the results' sums are numpy's."""
    nops = pkg._lib.LANE_SELFTEST_OPS
    assert nops == 32
    with np.errstate(over="ignore"):
        want = _expected_sums(U64(SEED))
    assert len(want) == nops
    bad, sums = pkg._lib.selftest_lane_ops(0, SEED)
    print("mismatching lanes:", bad)
    assert bad == [0] * nops
    assert sums == want, [k for k in range(nops) if sums[k] != want[k]]
    # (the check has teeth: distinct operations give distinct sums on this data)
    assert len(set(want)) > nops // 2


@pytest.fixture(scope="module")
def shape(pkg, oracle):
    g = drv.overlay(pkg, oracle)
    assert int(np.diff(g.row_ptr).max()) > drv.HUB_THRESHOLD   # k_hub_partial / k_hub_final run
    return g


_cache = {}


def _case(pkg, oracle, g, words):
    """(origin, oracle reference) of one width: computed once, never modified."""
    if words not in _cache:
        origin = drv.messages(pkg, g, drv.WIDTHS[words])
        ref = oracle.run(g, origin, None, nthreads=16)
        for a in drv.OUTPUTS:
            ref[a].setflags(write=False)
        _cache[words] = origin, ref
    return _cache[words]


def _engine_run(pkg, monkeypatch, g, origin, hub_threshold):
    env = {}
    drv.set_env(env)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return drv.run(pkg, g, origin, hub_threshold)


@pytest.mark.parametrize("words", sorted(drv.WIDTHS, reverse=True))
def test_commit_path_at_every_width(pkg, oracle, shape, monkeypatch, words):
    """seen, digest, coverage, forwards and every protocol counter of every
    round equal the oracle's at W = 64, 32, 16, 8, and the rounds' scan modes
    and done_nb / aliased counters show that the converted paths ran."""
    g = shape
    origin, ref = _case(pkg, oracle, g, words)
    run = _engine_run(pkg, monkeypatch, g, origin, drv.HUB_THRESHOLD)
    print(_work(run))
    _check_oracle(run, ref)
    st = run["stats"]
    nm = g.n * drv.WIDTHS[words]
    held = np.concatenate([[0], np.cumsum([s["new_bits"] + s["injected"] for s in ref["stats"]])])
    # done in-neighbours: dnb_pairs / dnb_quads (W = 64), dnb_groups (narrower rows)
    assert any(s["done_nb"] > 0 for s in st), "no done-neighbour receiver"
    if words == 64:
        # the plain early-exit pull before half the bits are held: the serial
        # loop with the packed gather (GP_LINE_PACK=1)
        assert any(s["scan"] == 2 and held[r] * 2 < nm <= ref["stats"][r - 1]["new_bits"] * 16
                   for r, s in enumerate(st) if r > 0), "no plain early-exit pull"
        # the first aliasing round (no done probe yet): the quads variant, whose
        # receivers of in-degree <= 32 go through gather_pairs
        assert any(s["scan"] == 2 and held[r] * 2 >= nm for r, s in enumerate(st)), "no first aliasing round"
        assert any(s["aliased"] > 0 for s in st), "no receiver aliased"
        assert any(s["scan"] & 64 for s in st), "no done-probe round"
    else:
        assert all(s["aliased"] == 0 for s in st)


def test_on_against_off(pkg, oracle, shape, monkeypatch, tmp_path):
    """The W = 64 case with the GP_LANE_OPS=0 build (child process, GOSSIP_HIP_LIB):
    equal in every output and every counter.  With the hub split the three work
    counters of the hub chunks' early-exit rounds depend on wave timing
    (csrc/hub.hip), so the run is repeated without hubs, where every counter is
    deterministic and compared."""
    import importlib
    sys.path.insert(0, os.path.dirname(pkg._lib.__file__))
    off_lib = importlib.import_module("build_lib").LANE_OFF_LIB
    assert os.path.exists(off_lib), "run __graft_entry__.build()"
    assert os.path.realpath(off_lib) != os.path.realpath(pkg._lib.load()._name)
    out = str(tmp_path / "off.npz")
    env = dict(os.environ, GOSSIP_HIP_LIB=off_lib)
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "lane_ops_driver.py"), out], env=env,
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-4000:]
    off = np.load(out)
    assert str(off["lib"]) == off_lib
    g = shape
    origin, _ = _case(pkg, oracle, g, 64)
    for tag, thr, drop in (("hub", drv.HUB_THRESHOLD, drv.TIMING_KEYS), ("flat", int(np.diff(g.row_ptr).max()) + 1, ())):
        on = _engine_run(pkg, monkeypatch, g, origin, thr)
        for k in drv.OUTPUTS:
            assert np.array_equal(on[k], off[f"{tag}_{k}"]), (tag, k)
        keys, mat = drv.counters(on["stats"])
        assert keys == list(off[f"{tag}_keys"])
        assert set(STAT_KEYS) <= set(keys) and set(drv.TIMING_KEYS) <= set(keys)
        keep = [i for i, k in enumerate(keys) if k not in drop]
        diff = np.argwhere(mat[:, keep] != off[f"{tag}_counters"][:, keep])
        assert diff.size == 0, [(int(r), keys[keep[int(c)]]) for r, c in diff]
