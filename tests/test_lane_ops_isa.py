"""Register budgets of the W = 64 pull variants after the move of their
cross-lane reductions from LDS shuffles to csrc/lane_ops.h.

CPU test, needs only hipcc: csrc/pull.hip is compiled to gfx950 assembly the
way scripts/isa_diff.py expects it (build_lib.FLAGS + `--cuda-device-only -S`)
and the variants a C4 run launches are read from it.  A check of register
budgets and of the change having happened, nothing else.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gossip-protocol-with-power-law_amd")

# k_expand<64, MODE>: (VGPRs before the change, arbitrary-lane reads left).
# A read of an arbitrary lane is not a reduction and stays a ds_bpermute_b32:
# each receiver group's `__shfl(slot_of, ks)` -- its receiver's slot byte, the
# lane differing per half / quarter of the wave.
VARIANTS = {
    3: (70, 2),     # SCAN_PRE (round 1): pre_quads and dnb_pairs, one each
    32: (62, 1),    # SCAN_FILTERED | SCAN_LINES (round 2): dnb_pairs
    514: (70, 1),   # SCAN_UNFILTERED | SCAN_PACK (round 3): dnb_pairs
    258: (72, 2),   # SCAN_UNFILTERED | SCAN_QUADS (round 4): dnb_quads and gather_pairs
    66: (70, 1),    # SCAN_UNFILTERED | SCAN_DPROBE (round 5): dnb_quads
    192: (68, 1),   # SCAN_FILTERED | SCAN_DPROBE | SCAN_LIST (late rounds): dnb_quads
}


def _symbol(mode):
    return f"_ZN2gp8k_expandILi64ELi{mode}EEEvNS_10ExpandArgsE"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    sys.path.insert(0, PKG)
    try:
        import build_lib
    finally:
        sys.path.remove(PKG)
    out = str(tmp_path_factory.mktemp("isa") / "pull.s")
    cmd = [build_lib._hipcc(), *build_lib.FLAGS, "--cuda-device-only", "-S", os.path.join(build_lib.CSRC, "pull.hip"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


def _metadata(asm, sym):
    """the kernel's entry of .amdgpu_metadata"""
    entries = re.split(r"^  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):], flags=re.M)
    mine = [e for e in entries if re.search(rf"^\s+\.name:\s+{re.escape(sym)}\s*$", e, re.M)]
    assert len(mine) == 1, sym
    return {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)\s*$", mine[0], re.M)}


def _code(asm, sym):
    """the kernel's instructions, comments stripped"""
    body = asm[asm.index(f"\n{sym}:"):]
    body = body[:body.index(".end_amdhsa_kernel")]
    return [l.split(";")[0].strip() for l in body.split("\n")]


@pytest.mark.parametrize("mode", sorted(VARIANTS))
def test_variant_budget(asm, mode):
    vgprs_before, lane_reads = VARIANTS[mode]
    sym = _symbol(mode)
    md = _metadata(asm, sym)
    code = _code(asm, sym)
    bperm = sum(1 for l in code if l.startswith("ds_bpermute_b32"))
    dpp = sum(1 for l in code if re.match(r"v_\w+_dpp\b", l))
    swaps = sum(1 for l in code if l.startswith("v_permlane"))
    print(f"k_expand<64, {mode}>: {md['vgpr_count']} VGPRs (before: {vgprs_before}), {md['sgpr_count']} SGPRs, "
          f"scratch {md['private_segment_fixed_size']}, ds_bpermute_b32 {bperm}, dpp {dpp}, swaps {swaps}")
    assert md["vgpr_count"] <= vgprs_before
    assert md["private_segment_fixed_size"] == 0
    assert bperm <= lane_reads
    assert dpp > 0 and swaps > 0   # the reductions are there, in the VALU
