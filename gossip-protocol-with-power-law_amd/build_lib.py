"""Build libgossip_hip.so for gfx950 in-tree (csrc/ -> _build/).

hipcc cross-compiles without a GPU, so this runs in the CPU container; the
built .so travels to the GPU box with the repo snapshot.
"""
import os
import subprocess
import sys

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
OUT_DIR = os.path.join(PKG_DIR, "_build")
LIB = os.path.join(OUT_DIR, "libgossip_hip.so")
INCLUDE = os.path.join(os.path.dirname(PKG_DIR), "include", "gossip_capi.h")
# every unit and header of csrc/ (the headers drive the staleness check)
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))
ARCH = os.environ.get("GOSSIP_OFFLOAD_ARCH", "gfx950")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result", f"--offload-arch={ARCH}"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    return "hipcc"


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


STANDIN_SRC = os.path.join(os.path.dirname(PKG_DIR), "tests", "native", "rccl_standin.cpp")
STANDIN_LIB = os.path.join(OUT_DIR, "libgossip_hip_rccl_standin.so")


def build_standin(force=False, verbose=True):
    """TEST build: the engine's own objects linked against the in-process RCCL
    stand-in of tests/native/rccl_standin.cpp instead of librccl, so the vertex
    partition's RCCL path (exchange_rccl) runs with P > 1 ranks as threads of
    one process on one GPU (tests/test_rccl_standin.py).  The product library
    (libgossip_hip.so) is not touched."""
    build(force=force, verbose=verbose)
    objs = [os.path.join(OUT_DIR, os.path.splitext(s)[0] + ".o") for s in SOURCES]
    if not force and not _stale(STANDIN_LIB, objs + [STANDIN_SRC, __file__]):
        return STANDIN_LIB
    sobj = os.path.join(OUT_DIR, "rccl_standin.o")
    cmd = [_hipcc(), "-O2", "-std=c++17", "-fPIC", "-Wall", f"--offload-arch={ARCH}", "-c", STANDIN_SRC, "-o", sobj]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    tmp = STANDIN_LIB + ".tmp"
    cmd = [_hipcc(), *FLAGS, "-shared", *objs, sobj, "-o", tmp, "-pthread"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, STANDIN_LIB)
    return STANDIN_LIB


LANE_OFF_UNITS = ("pull.hip", "hub.hip")   # the units GP_LANE_OPS changes (csrc/lane_ops.h)
LANE_OFF_LIB = os.path.join(OUT_DIR, "libgossip_hip_lane_off.so")


def build_lane_off(force=False, verbose=True):
    """TEST build: the engine with GP_LANE_OPS=0 -- the pull family's cross-lane
    reductions through LDS shuffles instead of csrc/lane_ops.h -- for the
    on-against-off case of tests/test_gpu_lane_ops.py and for A/B runs.  Only
    the units the knob changes are compiled again; the product library is not
    touched."""
    build(force=force, verbose=verbose)
    deps = [os.path.join(CSRC, s) for s in list(LANE_OFF_UNITS) + HEADERS] + [INCLUDE, LIB, __file__]
    if not force and not _stale(LANE_OFF_LIB, deps):
        return LANE_OFF_LIB
    objs, procs = [], []
    for s in SOURCES:
        stem = os.path.splitext(s)[0]
        if s not in LANE_OFF_UNITS:
            objs.append(os.path.join(OUT_DIR, stem + ".o"))
            continue
        obj = os.path.join(OUT_DIR, stem + ".lane_off.o")
        objs.append(obj)
        cmd = [_hipcc(), *FLAGS, "-DGP_LANE_OPS=0", "-c", os.path.join(CSRC, s), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append(subprocess.Popen(cmd))
    for p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed")
    tmp = LANE_OFF_LIB + ".tmp"
    cmd = [_hipcc(), *FLAGS, "-shared", *objs, "-o", tmp, "-lrccl", "-pthread"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, LANE_OFF_LIB)
    return LANE_OFF_LIB


def build(force=False, verbose=True):
    os.makedirs(OUT_DIR, exist_ok=True)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [INCLUDE, __file__]
    if not force and not _stale(LIB, deps):
        return LIB
    objs, procs = [], []
    for s in SOURCES:
        obj = os.path.join(OUT_DIR, os.path.splitext(s)[0] + ".o")
        objs.append(obj)
        cmd = [_hipcc(), *FLAGS, "-c", os.path.join(CSRC, s), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append(subprocess.Popen(cmd))
    for p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed")
    tmp = LIB + ".tmp"
    cmd = [_hipcc(), *FLAGS, "-shared", *objs, "-o", tmp, "-lrccl", "-pthread"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, LIB)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    build_standin(force="--force" in sys.argv)
    build_lane_off(force="--force" in sys.argv)
