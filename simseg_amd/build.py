"""Builds libsimseg_hip.so (gfx950 only) in-tree with hipcc.  `python -m simseg_amd.build`"""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsimseg_hip.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wno-unused-result"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


TWICE = ()     # sources compiled once per 16-bit type: none any more
# Every source is ONE object.  Where a kernel touches 16-bit data it takes the type (bf16 or fp16) as a template argument, picked per call
# from g_ss_half (csrc/common.h: with_h16); fp32 / integer code has no 16-bit type at all.


def build(force=False, verbose=True, always=(), report=None):
    """always: source basenames recompiled even when their object is current (the driver's build check: prove that hipcc cross-compiles
    here instead of finding everything prebuilt); report: a list that receives (source, object, 'compiled' | 'reused')."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    hdrs = sorted(glob.glob(os.path.join(CSRC, "*.h"))) + sorted(glob.glob(os.path.join(HERE, "..", "include", "*.h")))
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    objs, procs = [], []
    for s in srcs:
        o = os.path.join(objdir, os.path.basename(s)[:-4] + ".o")
        objs.append(o)
        fresh = force or _stale(o, [s] + hdrs) or os.path.basename(s) in always
        if report is not None:
            report.append((os.path.basename(s), os.path.basename(o), "compiled" if fresh else "reused"))
        if fresh:
            cmd = [hipcc] + FLAGS + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((s, subprocess.Popen(cmd)))
    for s, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {s}")
    for o in set(glob.glob(os.path.join(objdir, "*.o"))) - set(objs):      # objects of sources that are gone
        os.remove(o)
    if force or procs or _stale(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
