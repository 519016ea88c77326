#!/usr/bin/env python3
"""Many small pair alignments: ONE align_many call against the same jobs one after the other through one reused handle (GPU box).

    python tools/time_many.py [--jobs 10000] [--lmin 50] [--lmax 1000] [--reps 5] [--minlength 20] [--wave-max N] [--only loop|many] [--check]

Workload: J jobs of 2 x L bases, L uniform in lmin .. lmax, 1 % substitutions.  The two sides run alternately, `reps` times each:
  loop   rv_reset, rv_add_sample / rv_add_sequence x 2, rv_construct, rv_align_builtin, rv_fetch_anchors, the text -- per job, straight at
         the C ABI (no Python object per job); with RV_LIB_DIR set this side runs on another build of the libraries (the parent commit's)
  many   reveal_amd.many: Batch.add x J, run, anchors (the C part), and align_many as a whole (with the Python result lists)
Prints medians, the loop's spread, the ratio and one JSON line.  --check compares the two sides' anchors job by job."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reveal_amd import _lib, reveallib      # noqa: E402


def workload(jobs, lmin, lmax, seed=1):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for _ in range(jobs):
        L = int(rng.integers(lmin, lmax + 1))
        a = rng.integers(0, 4, L)
        b = a.copy()
        hit = rng.random(L) < 0.01
        b[hit] = (b[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        out.append([lut[a].tobytes(), lut[b].tobytes()])
    return out


def run_loop(idx, jobs, minl):
    """the jobs one after the other through one handle; -> per job sorted [(l, (a, b))]"""
    dll, h = idx._dll, idx._h
    st = _lib.RvAlignStats()
    mem = ctypes.c_int64(0)
    res = []
    for a, b in jobs:
        ok = dll.rv_reset(h) == 0
        for s in (a, b):
            ok = ok and dll.rv_add_sample(h) == 0 and dll.rv_add_sequence(h, s, len(s), None, None) == 0
        ok = ok and dll.rv_construct(h, 0, None, None, 0) == 0 and dll.rv_align_builtin(h, minl, 2, ctypes.byref(st)) == 0
        if not ok:
            raise RuntimeError(idx._lib.err())
        na = dll.rv_anchor_count(h, ctypes.byref(mem))
        l = np.empty(max(na, 1), np.uint32); off = np.empty(na + 1, np.int64); pos = np.empty(max(mem.value, 1), np.int64)
        off[0] = 0
        n = len(a) + len(b) + 2
        T = ctypes.create_string_buffer(n)
        if dll.rv_fetch_anchors(h, l.ctypes.data, off.ctypes.data, pos.ctypes.data) != 0 or dll.rv_get_array(h, _lib.RV_T, T, n) != n:
            raise RuntimeError(idx._lib.err())
        res.append((l[:na], pos[:2 * na]))
    return res


def run_many_c(batch, jobs, minl):
    batch.clear()
    for j in jobs:
        batch.add(j)
    batch.run(minl, 2)
    return batch.anchors()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=10000)
    ap.add_argument("--lmin", type=int, default=50)
    ap.add_argument("--lmax", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--minlength", type=int, default=20)
    ap.add_argument("--wave-max", type=int, default=None)
    ap.add_argument("--only", choices=("loop", "many"), default=None)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    jobs = workload(a.jobs, a.lmin, a.lmax)
    bases = sum(len(x) + len(y) for x, y in jobs)
    t_loop, t_many, t_many_py = [], [], []
    idx = reveallib.index() if a.only != "many" else None
    batch = None
    if a.only != "loop":
        from reveal_amd import many      # (not needed by --only loop: that side also runs from a checkout without the module)
        batch = many.Batch(False)
        if a.wave_max is not None:
            batch.option("RV_MANY_WAVE_MAX", a.wave_max)
        run_many_c(batch, jobs[:64], a.minlength)      # (first use: allocations, code objects)
    if idx is not None:
        run_loop(idx, jobs[:64], a.minlength)
    loop_res = many_res = None
    for rep in range(a.reps):
        if idx is not None:
            t = time.perf_counter(); loop_res = run_loop(idx, jobs, a.minlength); t_loop.append(time.perf_counter() - t)
        if batch is not None:
            t = time.perf_counter(); many_res = run_many_c(batch, jobs, a.minlength); t_many.append(time.perf_counter() - t)
            t = time.perf_counter(); many.align_many(jobs, a.minlength, 2, toupper=False, batch=batch); t_many_py.append(time.perf_counter() - t)
    out = dict(jobs=a.jobs, lmin=a.lmin, lmax=a.lmax, bases=bases, minlength=a.minlength, reps=a.reps, lib_dir=os.environ.get("RV_LIB_DIR", ""))
    if t_loop:
        out.update(loop_s=t_loop, loop_median_s=statistics.median(t_loop), loop_spread_s=max(t_loop) - min(t_loop),
                   loop_jobs_per_s=a.jobs / statistics.median(t_loop))
        print("loop  : median %.3f s (min %.3f, max %.3f: spread %.3f s), %.0f jobs/s" % (out["loop_median_s"], min(t_loop), max(t_loop), out["loop_spread_s"], out["loop_jobs_per_s"]))
    if t_many:
        out.update(many_s=t_many, many_median_s=statistics.median(t_many), many_jobs_per_s=a.jobs / statistics.median(t_many),
                   align_many_median_s=statistics.median(t_many_py), info=batch.info())
        print("many  : median %.3f s (min %.3f, max %.3f), %.0f jobs/s; align_many with its Python result lists: median %.3f s; %r"
              % (out["many_median_s"], min(t_many), max(t_many), out["many_jobs_per_s"], out["align_many_median_s"], out["info"]))
    if t_loop and t_many:
        out["ratio"] = out["loop_median_s"] / out["many_median_s"]
        out["gain_s"] = out["loop_median_s"] - out["many_median_s"]
        print("ratio : %.1f x  (gain %.3f s against a spread of %.3f s)" % (out["ratio"], out["gain_s"], out["loop_spread_s"]))
    if a.check and loop_res is not None and many_res is not None:
        first, l, off, pos = many_res
        bad = 0
        for j, (ll, lp) in enumerate(loop_res):
            lo, hi = int(first[j]), int(first[j + 1])
            got = sorted((int(l[k]), int(pos[2 * k]), int(pos[2 * k + 1])) for k in range(lo, hi))
            ref = sorted((int(ll[k]), int(lp[2 * k]), int(lp[2 * k + 1])) for k in range(len(ll)))
            bad += got != ref
        out["check_bad_jobs"] = bad
        print("check : %d of %d jobs differ between the two sides" % (bad, a.jobs))
    print(json.dumps(out))
    return 1 if out.get("check_bad_jobs") else 0


if __name__ == "__main__":
    sys.exit(main())
