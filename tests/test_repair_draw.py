"""The partner draw of anti-entropy repair (csrc/repair_draw.h) on the CPU.

k_repair_offer (csrc/repair.hip) picks with this header the one in-neighbour
whose Message-List a peer pulls in a repair round.  The test compiles the
header with g++ through tests/native/repair_draw_shim.cpp and compares it with
the package's numpy twin (repair.partner_index) and with the reference's own
copy (tests/repair_ref.py) on random (seed, r, v, deg), in-degree 1 and
in-degrees of 2^20 and more included, then checks that the index is uniform."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import repair_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip-protocol-with-power-law_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "native", "repair_draw_shim.cpp")


@pytest.fixture(scope="module")
def rd(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("repair_draw") / "librepair_draw_shim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, SHIM,
                           "-o", so])
    lib = ctypes.CDLL(so)
    lib.rd_stream.restype = ctypes.c_ulonglong
    lib.rd_round_key.argtypes = [ctypes.c_ulonglong, ctypes.c_uint]
    lib.rd_round_key.restype = ctypes.c_ulonglong
    lib.rd_partner_index.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_longlong]
    lib.rd_partner_index.restype = None
    return lib


def native_index(rd, seed, r, v, deg):
    v = np.ascontiguousarray(v, np.uint64)
    deg = np.ascontiguousarray(np.broadcast_to(np.asarray(deg, np.uint64), v.shape))
    seed = np.ascontiguousarray(np.broadcast_to(np.asarray(seed, np.uint64), v.shape))
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(r, np.uint32), v.shape))
    out = np.zeros(v.size, np.uint64)
    rd.rd_partner_index(seed.ctypes.data, r.ctypes.data, v.ctypes.data, deg.ctypes.data, out.ctypes.data, v.size)
    return out.astype(np.int64)


def test_constants_and_rounds(pkg, rd):
    assert rd.rd_stream() == 0x400 == pkg.repair.STREAM_REPAIR == repair_ref.STREAM_REPAIR
    assert rd.rd_period_max() == 64 == pkg.repair.PERIOD_MAX
    for period in (1, 2, 3, 4, 7, 64):
        want = [(r + 1) % period == 0 for r in range(254)]
        assert [bool(rd.rd_repair_round(r, period)) for r in range(254)] == want
        assert [pkg.repair.is_repair_round(r, period) for r in range(254)] == want
        assert [repair_ref.is_repair_round(r, period) for r in range(254)] == want
        assert sum(want[:period]) == 1 and want[period - 1]   # every window of `period` rounds holds one
    assert not rd.rd_repair_round(5, 0) and not pkg.repair.is_repair_round(5, 0) and not repair_ref.is_repair_round(5, 0)
    assert not pkg.repair.is_repair_round(5, None)


def test_round_key(pkg, rd, harness):
    for seed, r in ((0, 0), (21, 7), ((1 << 64) - 1, 253)):
        key = harness.splitmix64(seed ^ harness.splitmix64(0x400 + r))
        assert rd.rd_round_key(seed, r) == key == pkg.repair.round_key(seed, r)


def test_three_copies_agree(pkg, rd, harness):
    rng = np.random.default_rng(23)
    k = 100_000
    seeds = rng.integers(0, 1 << 63, 8, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 8, dtype=np.uint64)
    rounds = np.array([0, 1, 7, 100, 253], np.uint32)
    v = rng.integers(0, 1 << 32, k, dtype=np.uint64)
    # in-degrees: 1, small ones, around 2^20, up to 2^32 - 1
    deg = np.concatenate([np.ones(k // 4, np.uint64), rng.integers(2, 1000, k // 4, dtype=np.uint64),
                          rng.integers(1 << 20, 1 << 21, k // 4, dtype=np.uint64),
                          rng.integers(1 << 21, 1 << 32, k - 3 * (k // 4), dtype=np.uint64)])
    deg[-1] = (1 << 32) - 1
    si, ri = rng.integers(0, seeds.size, k), rng.integers(0, rounds.size, k)
    got = native_index(rd, seeds[si], rounds[ri], v, deg)
    assert (got >= 0).all() and (got < deg.astype(np.int64)).all() and (got[deg == 1] == 0).all()
    assert (got[deg >= 1 << 20] >= 1 << 16).mean() > 0.9   # (the high word of the product is used)
    for a in range(seeds.size):
        for b in range(rounds.size):
            sel = (si == a) & (ri == b)
            want = pkg.repair.partner_index(int(seeds[a]), int(rounds[b]), v[sel], deg[sel])
            assert np.array_equal(got[sel], want)
            assert np.array_equal(want, repair_ref.partner_index(int(seeds[a]), int(rounds[b]), v[sel], deg[sel]))
    for i in list(range(10)) + list(range(k - 10, k)):   # a few by the oracle harness's scalar draw
        d = harness.draw(int(seeds[si[i]]), 0x400 + int(rounds[ri[i]]), int(v[i]))
        assert int(got[i]) == (d * int(deg[i])) >> 64
        assert int(got[i]) == repair_ref.partner_index_int(int(seeds[si[i]]), int(rounds[ri[i]]), int(v[i]), int(deg[i]))
    with pytest.raises(ValueError):
        pkg.repair.partner_index(1, 0, [3], [0])


def test_partners_of_a_csr(pkg, rd):
    """partners(): the column at the drawn index, -1 without an in-neighbour; the numpy twin and the reference agree"""
    g = pkg.CSR.from_arcs(6, [0, 1, 2, 2, 4], [1, 2, 1, 3, 2], directed=True)
    rp, col = np.asarray(g.row_ptr), np.asarray(g.col)
    for r in (0, 3, 9):
        got = pkg.repair.partners(g, 21, r)
        assert np.array_equal(got, repair_ref.partners(g, 21, r))
        for v in range(6):
            deg = int(rp[v + 1] - rp[v])
            if deg == 0:
                assert got[v] == -1
            else:
                assert got[v] == col[rp[v] + native_index(rd, 21, r, [v], deg)[0]]
    assert got[0] == -1 and got[5] == -1 and got[3] == 2


@pytest.mark.parametrize("deg", [2, 3, 8, 913])
def test_index_is_uniform(pkg, deg):
    """10^6 vertices: every index's share within 5 binomial standard deviations of 1 / deg"""
    k = 1_000_000
    idx = pkg.repair.partner_index(21, 5, np.arange(k), deg)
    share = np.bincount(idx, minlength=deg) / k
    sd = np.sqrt((1 / deg) * (1 - 1 / deg) / k)
    assert np.abs(share - 1 / deg).max() <= 5 * sd
    # another round draws other partners
    assert (idx != pkg.repair.partner_index(21, 6, np.arange(k), deg)).mean() > 0.4
