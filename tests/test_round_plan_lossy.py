"""The planner's rule for lossy links (csrc/round_plan.h) on
the CPU: RoundFacts::lossy set gives PULL_LOSSY and nothing else -- no push and
every switch false, whatever the other facts say, because each shortcut of the
flood rests on "a neighbour's whole Message-List was sent to me" -- and with
the flag clear the plan is the one a RoundFacts without the field gets
(tests/native/round_plan_shim.cpp, which never names it).  Over every
combination of the boolean facts, W in {1, 8, 16, 32, 64}, and three stages of
a run (sparse start, dense middle, nearly done)."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from test_round_plan import BASE, CSRC, FACTS, FLAGS, PLAN, ROOT, SHIM

LOSSY_SHIM = os.path.join(ROOT, "tests", "native", "round_plan_lossy_shim.cpp")
BOOLS = ("local liveness_active alive_on alive_now have_cml have_lm have_lmw have_ldone have_ld_cand can_park "
         "can_list cml_written lm_written alias_active ulist_valid park_failed").split()
# (prev_new_bits, prev_receivers, prev_next_arcs, held_bits) as shares of n * m, n, nnz, n * m
STAGES = [(0.0001, 0.002, 0.001, 0.0002), (0.2, 0.95, 0.9, 0.3), (0.01, 0.3, 0.2, 0.97)]


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("round_plan_lossy")
    out = []
    for src, name in ((SHIM, "plain"), (LOSSY_SHIM, "lossy")):
        so = str(d / f"lib{name}.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, src,
                               "-o", so])
        out.append(ctypes.CDLL(so))
    plain, lossy = out
    plain.rp_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    plain.rp_plan.restype = None
    lossy.rpl_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    lossy.rpl_plan.restype = None
    lossy.rpl_pull_lossy.restype = ctypes.c_longlong
    return plain, lossy


def fact_blocks():
    """one block per (W, configuration, stage): every combination of BOOLS"""
    combos = np.array(list(itertools.product((0, 1), repeat=len(BOOLS))), np.int64)
    for W, m in ((1, 64), (8, 512), (16, 1000), (32, 2048), (64, 4096)):
        for push_ratio, compact_rows in ((0.0, 1), (0.0, 0), (10.0, 0)):
            for stage in STAGES:
                f = np.zeros(len(combos), FACTS)
                for k, v in BASE.items():
                    f[k] = v
                f["words"], f["m"], f["push_ratio"], f["compact_rows"] = W, m, push_ratio, compact_rows
                f["arc_mask_permille"] = 10
                nm = int(f["n"][0]) * m
                f["prev_new_bits"] = int(stage[0] * nm)
                f["prev_receivers"] = int(stage[1] * f["n"][0])
                f["prev_next_arcs"] = int(stage[2] * f["nnz"][0])
                f["held_bits"] = int(stage[3] * nm)
                f["ulist_n"], f["sate_since"] = 50, 1
                for j, name in enumerate(BOOLS):
                    f[name] = combos[:, j]
                yield np.ascontiguousarray(f)


def test_lossy_plans(libs):
    plain, lossy = libs
    pull_lossy = lossy.rpl_pull_lossy()
    kernels, flags, blocks = set(), set(), 0
    for facts in fact_blocks():
        n = facts.size
        blocks += 1
        ref = np.zeros(n, PLAN)
        plain.rp_plan(facts.ctypes.data, ref.ctypes.data, n)
        kernels |= set(np.unique(ref["kernel"]).tolist())
        flags |= {k for k in FLAGS if ref[k].any()}

        off, clear, flag = np.zeros(n, PLAN), np.zeros(n, np.int64), np.ones(n, np.int64)
        lossy.rpl_plan(facts.ctypes.data, clear.ctypes.data, off.ctypes.data, n)
        assert off.tobytes() == ref.tobytes()   # flag clear: bit for bit the plan without the field

        on = np.zeros(n, PLAN)
        lossy.rpl_plan(facts.ctypes.data, flag.ctypes.data, on.ctypes.data, n)
        assert (on["kernel"] == pull_lossy).all()
        for k in FLAGS + ["mode", "k_masked", "k_lines", "k_lm_from_commits", "need_park_slot", "need_ulist", "scan"]:
            assert not on[k].any(), k
    assert blocks == 5 * 3 * 3
    # the sweep is no empty one: pushes and pulls of every other kernel, most switches
    assert pull_lossy not in kernels and len(kernels) >= 4, kernels
    assert "mode_push" in flags and len(flags) >= 15, flags
