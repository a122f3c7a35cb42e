"""The recorded runs behind tests/golden/round_plan_trace.json: per-round
records (gp_round_stats without the *_ms timings) of five small runs, with
what csrc/round_plan.h's planner needs to replay them on the CPU (sizes, the
whole configuration, each round's injection).

    python tests/round_trace.py OUT.json        # record all five with the library in use

tests/test_gpu_pull_schedule.py runs (a)-(d) again and compares them with the
fixture field by field; tests/test_round_plan.py replays all five through the
planner without a GPU.  The fixture was recorded with the library of the
commit before the planner existed, so both compare against that commit.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "round_plan_trace.json")
N_WIDE = 60_000

# name -> (messages, configuration on top of the base, environment at gp_create)
BASE = dict(track_first=1, track_digest=1, track_msg_forwards=0, churn=0, p_fail=0.0, churn_seed=0,
            hub_threshold=64, push_ratio=0.0, unfiltered_pct=90, flat_max_words=16, arc_mask_permille=0,
            prefilter_pct=20, compact_rows=0)
RUNS = {
    "a": (4096, {}, {}),
    "b": (4096, dict(churn=1, p_fail=0.01, churn_seed=5), {}),
    "c": (512, dict(push_ratio=None), {}),   # None: the library's default
    "d": (4096, dict(compact_rows=1), {}),
    "e": (4096, {}, {"GP_LINE_DONE": "1", "GP_LINE_PACK": "1"}),
}


def overlay(pkg, oracle):
    """the `wide` overlay of tests/test_gpu_pull_schedule.py and its 4096 messages"""
    rp, col = oracle.chung_lu(N_WIDE, 12, 2.4, 43)
    g = pkg.CSR(N_WIDE, rp, col, False)
    origin = np.repeat(pkg.overlay.random_origins(g.n, 512, seed=43), 8).astype(np.int32)
    return g, origin


def run_cfg(name):
    cfg = dict(BASE)
    cfg.update(RUNS[name][1])
    return {k: v for k, v in cfg.items() if v is not None}


def record(pkg, g, origin, name):
    """One run on the GPU: the fixture entry of run `name` (its environment
    must already be set: it is read at gp_create)."""
    m = RUNS[name][0]
    origin = origin[:m]
    deg = np.diff(g.row_ptr)
    uniq = np.unique(origin)   # every message is injected in round 0
    with pkg.GossipEngine(0, **run_cfg(name)) as eng:
        eng.load_graph(g)
        eng.set_messages(origin)
        eng.reset()
        stats = eng.run()
        cfg = {f[0]: getattr(eng.cfg, f[0]) for f in eng.cfg._fields_}
    return dict(name=name, n=int(g.n), nnz=int(g.col.size), m=int(m), cfg=cfg, env=RUNS[name][2],
                inj_arcs=[int(deg[uniq].sum())], inj_groups=[int(uniq.size)],
                rounds=[{k: v for k, v in s.items() if not k.endswith("_ms")} for s in stats])


def main(out, only=None):
    sys.path.insert(0, ROOT)
    import _gossip_pkg
    from oracle import lib as oracle
    oracle.load()
    pkg = _gossip_pkg.load()
    g, origin = overlay(pkg, oracle)
    if only:   # the child process of a run with an environment of its own
        json.dump(record(pkg, g, origin, only), open(out, "w"))
        return
    entries = []
    for name, (_, _, env) in RUNS.items():
        if env:   # (the environment is read at gp_create: a fresh process)
            subprocess.run([sys.executable, os.path.abspath(__file__), out + "." + name, name],
                           env=dict(os.environ, **env), check=True, timeout=120)
            entries.append(json.load(open(out + "." + name)))
            os.remove(out + "." + name)
        else:
            entries.append(record(pkg, g, origin, name))
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in entries) + "\n]\n")
    for e in entries:
        print(e["name"], [(r["mode"], r["scan"]) for r in e["rounds"]], flush=True)


if __name__ == "__main__":
    main(*sys.argv[1:3])
