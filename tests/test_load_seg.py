"""Owner search and segment bookkeeping of the per-peer traffic pass
(csrc/load_seg.h, used by k_load of csrc/load.hip), on the CPU: the stand-alone
program tests/native/load_seg_check.cpp walks 64-receiver waves over rows of
every shape -- empty, short, exactly a chunk, long, hubs skipped or not, down
receivers, vertex counts around the wave size -- and compares each receiver's
sum with a row-by-row one.  What is summed is the per-peer total of the
arrivals each reference peer logs (Peer.py:206, Peer.py:286)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gossip-protocol-with-power-law_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "load_seg_check.cpp")


def test_wave_walk_matches_row_sums(tmp_path):
    exe = str(tmp_path / "load_seg_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "load_seg ok"
