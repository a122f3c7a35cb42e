"""DESIGN.md §3.1 / §3.9 against the sources: the compile-time knobs the table
names are the ones csrc/ defines, the build's file lists are the folder's
contents, and no unit outgrows the stated size."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gossip-protocol-with-power-law_amd")
CSRC = os.path.join(PKG, "csrc")


def _section(number):
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    m = re.search(rf"^### {re.escape(number)} .*?(?=^##)", text, re.M | re.S)
    assert m, f"DESIGN.md has no section {number}"
    return m.group(0)


def _csrc(ext):
    return sorted(f for f in os.listdir(CSRC) if f.endswith(ext))


def test_knob_table_matches_sources():
    found = []
    for f in _csrc(".hip") + _csrc(".h"):
        found += re.findall(r"^\s*#\s*ifndef\s+(GP_\w+)", open(os.path.join(CSRC, f), encoding="utf-8").read(), re.M)
    assert len(found) == len(set(found)), "a knob is defined twice"
    sec = _section("3.9")
    rows = [l for l in sec.splitlines() if l.startswith("| `GP_")]
    named = [k for l in rows for k in re.findall(r"`(GP_\w+)`", l.split("|")[1])]
    assert len(named) == len(set(named)), "a knob has two rows"
    assert set(found) - set(named) == set(), "knobs of csrc/ without a row in DESIGN.md §3.9"
    assert set(named) - set(found) == set(), "DESIGN.md §3.9 names knobs csrc/ does not define"
    stated = re.search(r"^(\d+) `#ifndef GP_\*` knobs", sec, re.M)
    assert stated, "DESIGN.md §3.9 no longer states the knob count"
    assert int(stated.group(1)) == len(found)


def test_build_lists_are_the_folder():
    sys.path.insert(0, PKG)
    try:
        import build_lib
    finally:
        sys.path.remove(PKG)
    assert sorted(build_lib.SOURCES) == _csrc(".hip")
    assert sorted(build_lib.HEADERS) == _csrc(".h")


def test_unit_sizes():
    # the limit is the one DESIGN.md §3.1 states
    stated = re.search(r"[Nn]o file under `csrc/` is over ([\d,]+) lines", _section("3.1"))
    assert stated, "DESIGN.md §3.1 no longer states the size limit"
    limit = int(stated.group(1).replace(",", ""))
    assert limit == 1400
    sizes = {f: sum(1 for _ in open(os.path.join(CSRC, f), encoding="utf-8")) for f in os.listdir(CSRC)}
    over = {f: n for f, n in sizes.items() if n > limit}
    assert not over, f"over {limit} lines: {over}"
