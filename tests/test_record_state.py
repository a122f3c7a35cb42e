"""The per-run records' lifecycle state (csrc/records.h), on the CPU.

Every record -- spread curve, traffic, fresh deliveries and their curve,
per-link fresh deliveries, receipt delays and their distributions, delivery
multiplicity, watched peers -- keeps three flags in the context (asked for /
in force / still valid) and moves them through the same four transitions;
gp_reset sizes the exact frontier rows for the mask of those who read them.
This test drives that plain-C++ part, compiled with g++ through a test-only
shim (tests/native/records_shim.cpp), over every combination of the flags
against a restatement in Python.  The records themselves aggregate what each
reference peer logs per arrival (Peer.py:175-216); their values are compared
with the references in the records' own test files.
"""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip-protocol-with-power-law_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "native", "records_shim.cpp")

WANT, ON, VALID = 1, 2, 4
# kRecords' order (csrc/records.h RecordId)
RECORDS = ("load", "curve", "fresh", "mult", "fresh_curve", "link", "delay", "delay_dist", "watch")


@pytest.fixture(scope="module")
def rs(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("records") / "librecords_shim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", CSRC, SHIM, "-o", so])
    lib = ctypes.CDLL(so)
    lib.rs_frx_mask.restype = ctypes.c_uint
    lib.rs_frx_mask.argtypes = [ctypes.c_int] * 4 + [ctypes.c_uint]
    return lib


def test_codes_and_count(rs, pkg):
    assert rs.rs_record_count() == len(RECORDS)
    assert rs.rs_enotrack() == pkg._lib.GP_ENOTRACK and rs.rs_estate() == pkg._lib.GP_ESTATE


@pytest.mark.parametrize("flags", range(8))
def test_take_effect_and_off(rs, flags):
    """gp_reset: on and valid become what is wanted now, the request stays"""
    want = flags & WANT
    assert rs.rs_take_effect(flags, 1) == want | ON | VALID
    assert rs.rs_take_effect(flags, 0) == want
    assert rs.rs_off(flags) == want


@pytest.mark.parametrize("flags", range(8))
def test_restored(rs, flags):
    """valid falls iff the record is on and the run is restored past round 0"""
    assert rs.rs_restored(flags, 0) == flags                         # a restore at round 0 keeps valid
    for r in (1, 2, 253):
        want = flags & ~VALID if flags & ON else flags              # off: nothing changes
        assert rs.rs_restored(flags, r) == want


def refusal(flags, partitioned, keeps_partition, state_ready, enotrack, estate):
    if partitioned and not keeps_partition:
        return enotrack
    if not flags & ON or not state_ready:
        return enotrack
    if not flags & VALID:
        return estate
    return 0


def test_refusal_precedence(rs):
    """partitioned before not-on (or no run state) before not-valid"""
    nt, st = rs.rs_enotrack(), rs.rs_estate()
    assert nt != 0 and st != 0 and nt != st
    for flags, part, keeps, ready in itertools.product(range(8), (0, 1), (0, 1), (0, 1)):
        assert rs.rs_refusal(flags, part, keeps, ready) == refusal(flags, part, keeps, ready, nt, st), (flags, part, keeps, ready)
    # the cases by name: a single-rank record, on but not valid, on a partitioned context
    assert rs.rs_refusal(ON, 1, 0, 1) == nt
    assert rs.rs_refusal(ON, 0, 0, 1) == st
    assert rs.rs_refusal(VALID, 0, 0, 1) == nt                      # not on, whatever valid says
    assert rs.rs_refusal(ON | VALID, 0, 0, 0) == nt                 # no run state
    # a record kept by partitioned contexts (delay, delay_dist, curve) is not refused on one
    assert rs.rs_refusal(ON | VALID, 1, 1, 1) == 0
    assert rs.rs_refusal(ON, 1, 1, 1) == st


def test_delay_rows_needed(rs):
    for dw, dd, uniform, force in itertools.product((0, 1), (0, 1), (-1, 0, 3), (0, 1)):
        assert rs.rs_delay_rows_needed(dw, dd, uniform, force) == int(bool(dw or dd) and (uniform < 0 or bool(force)))
    assert rs.rs_delay_rows_needed(1, 0, 0, 0) == 0                  # a one-round table needs no rows


def needs_of(rs, want, uniform, force):
    """the records' needs_frx hooks, restated: load reads no frontier rows, the
    two delay records read them for a table of several inject rounds, every
    other record whenever it is wanted"""
    w = dict(zip(RECORDS, want))
    rows = rs.rs_delay_rows_needed(w["delay"], w["delay_dist"], uniform, force)
    need = {k: bool(v) for k, v in w.items()}
    need["load"] = False
    need["delay"] = need["delay_dist"] = bool(rows)
    return sum(1 << k for k, name in enumerate(RECORDS) if need[name])


def test_frx_mask_one_bit_each(rs):
    r0 = rs.rs_record0()
    singles = [rs.rs_frx_mask(1, 0, 0, 0, 0), rs.rs_frx_mask(0, 1, 0, 0, 0), rs.rs_frx_mask(0, 0, 1, 0, 0),
               rs.rs_frx_mask(0, 0, 0, 1, 0)] + [rs.rs_frx_mask(0, 0, 0, 0, 1 << k) for k in range(len(RECORDS))]
    assert all(m != 0 and m & (m - 1) == 0 for m in singles)         # exactly one bit
    assert len(set(singles)) == len(singles)                         # its own
    assert [rs.rs_frx_mask(0, 0, 0, 0, 1 << k) for k in range(len(RECORDS))] == [1 << (r0 + k) for k in range(len(RECORDS))]
    assert rs.rs_frx_mask(0, 0, 0, 0, 0) == 0
    allm = rs.rs_frx_mask(1, 1, 1, 1, (1 << len(RECORDS)) - 1)
    assert allm == sum(singles)


def test_frx_mask_is_holds_frx(rs):
    """nonzero iff the expression Ctx::holds_frx() spelled out before the table"""
    n = 0
    for fwd, local, loss, lag, uniform, force in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (-1, 0), (0, 1)):
        for want in itertools.product((0, 1), repeat=len(RECORDS)):
            w = dict(zip(RECORDS, want))
            delay_needs_rows = bool(w["delay"] or w["delay_dist"]) and (uniform < 0 or bool(force))
            old = bool(fwd or local or w["curve"] or w["fresh"] or w["fresh_curve"] or w["link"] or delay_needs_rows or
                       w["mult"] or w["watch"] or loss or lag)
            mask = rs.rs_frx_mask(fwd, local, loss, lag, needs_of(rs, want, uniform, force))
            assert (mask != 0) == old, (fwd, local, loss, lag, uniform, force, w)
            n += 1
    assert n == 2 ** 15
    # delay wanted with a one-round table: no rows; with several inject rounds, or forced: rows
    only_delay = tuple(int(k == "delay") for k in RECORDS)
    assert rs.rs_frx_mask(0, 0, 0, 0, needs_of(rs, only_delay, 0, 0)) == 0
    assert rs.rs_frx_mask(0, 0, 0, 0, needs_of(rs, only_delay, -1, 0)) != 0
    assert rs.rs_frx_mask(0, 0, 0, 0, needs_of(rs, only_delay, 0, 1)) != 0
    only_load = tuple(int(k == "load") for k in RECORDS)
    assert rs.rs_frx_mask(0, 0, 0, 0, needs_of(rs, only_load, -1, 0)) == 0
