"""Lane mapping of the packed row gather (csrc/line_pack.h), on the CPU.

The early-exit pulls of 64-word rows gather only the 128-B lines on which the
receiver still misses messages; with one or two such lines the lanes of a
wave (or of a half-wave, where receivers go two at a time) are dealt out so
that a load instruction carries eight or four senders' rows instead of two.
The gather stays exact only if the mapping is a bijection between lanes and
the (row slot, 16-B piece) pairs of the live lines, so this test drives the
header, compiled with g++ through a test-only shim
(tests/native/line_pack_shim.cpp), over all 15 masks and every lane.  The
layout only schedules the loads: the OR over a receiver's in-neighbours, the
reference's send loop over every link (Peer.py:402-404), is the same whatever
lane loads which piece.
"""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip-protocol-with-power-law_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "native", "line_pack_shim.cpp")

MASKS = list(range(1, 16))


@pytest.fixture(scope="module")
def lp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("line_pack") / "libline_pack_shim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", CSRC, SHIM, "-o", so])
    lib = ctypes.CDLL(so)
    for name, n in (("count", 1), ("row_shift", 1), ("slot", 2), ("piece", 2), ("lane", 3)):
        f = getattr(lib, "lp_shim_" + name)
        f.argtypes = [ctypes.c_uint] + [ctypes.c_int] * (n - 1)
        f.restype = ctypes.c_int
    return lib


def lines(mask):
    return [l for l in range(4) if mask >> l & 1]


@pytest.mark.parametrize("mask", MASKS)
def test_rows_per_instruction(lp, mask):
    p = len(lines(mask))
    assert lp.lp_shim_count(mask) == p
    assert 1 << lp.lp_shim_row_shift(mask) == {1: 8, 2: 16, 3: 32, 4: 32}[p]


@pytest.mark.parametrize("width", [64, 32])   # a wave, a half-wave
@pytest.mark.parametrize("mask", MASKS)
def test_every_live_piece_has_one_lane(lp, mask, width):
    """Every (slot, piece) of a live line is taken by exactly one lane, no lane
    maps into a dead line, and the inverse returns the lane."""
    live = lines(mask)
    lanes_per_row = 1 << lp.lp_shim_row_shift(mask)
    slots = width // lanes_per_row
    taken = {}
    for lane in range(width):
        slot, piece = lp.lp_shim_slot(mask, lane), lp.lp_shim_piece(mask, lane)
        assert 0 <= slot < slots
        if piece < 0:
            continue
        assert 0 <= piece < 32 and piece >> 3 in live, (lane, piece)
        assert (slot, piece) not in taken, (lane, taken[(slot, piece)])
        taken[(slot, piece)] = lane
        assert lp.lp_shim_lane(mask, slot, piece) == lane
    assert set(taken) == {(s, 8 * l + q) for s in range(slots) for l in live for q in range(8)}
    # idle lanes only where the row layout leaves a dead line its lanes
    assert width - len(taken) == (slots * 8 if len(live) == 3 else 0)
    for s in range(slots):
        for piece in range(32):
            if piece >> 3 not in live:
                assert lp.lp_shim_lane(mask, s, piece) == -1


@pytest.mark.parametrize("mask", [m for m in MASKS if bin(m).count("1") >= 3])
def test_three_and_four_lines_keep_the_row_layout(lp, mask):
    """32 lanes per row, lane l of a row its piece l: gather_rows_n's layout."""
    for lane in range(64):
        assert lp.lp_shim_slot(mask, lane) == lane // 32
        want = lane % 32 if mask >> ((lane % 32) // 8) & 1 else -1
        assert lp.lp_shim_piece(mask, lane) == want


@pytest.mark.parametrize("mask", [m for m in MASKS if bin(m).count("1") <= 2])
def test_packed_lines_are_whole_octets(lp, mask):
    """A line is loaded by eight consecutive lanes in piece order (one 128-B
    request per octet), the lower line first."""
    live = lines(mask)
    for lane in range(64):
        octet = lane // 8 % len(live)
        assert lp.lp_shim_piece(mask, lane) == 8 * live[octet] + lane % 8
        assert lp.lp_shim_slot(mask, lane) == lane // (8 * len(live))


def test_a_half_wave_is_the_wave_layout_shifted(lp):
    """Half 1 of a wave maps as half 0 does, its slots behind half 0's."""
    for mask in MASKS:
        per_half = 32 >> lp.lp_shim_row_shift(mask)
        for lane in range(32):
            assert lp.lp_shim_piece(mask, lane + 32) == lp.lp_shim_piece(mask, lane)
            assert lp.lp_shim_slot(mask, lane + 32) == lp.lp_shim_slot(mask, lane) + per_half
