#!/usr/bin/env python3
"""Many small pair alignments: ONE align_many call against the same jobs one after the other through one reused handle (GPU box).

    python tools/time_many.py [--jobs 10000] [--lmin 50] [--lmax 1000] [--reps 5] [--minlength 20] [--wave-max N] [--only loop|many] [--check]
                              [--seqs K] [--multi 0|1|ab] [--large 0|1|ab] [--large-multi 0|1|ab] [--large-max R] [--large-min J]
                              [--wide 0|1|ab] [--wide-large-min J] [--no-cut] [--sites] [--picker [--rem-jobs N]]
                              [--chain-wide [--save-digests FILE] [--compare-digests FILE]] [--chain-wide-large [--chain-wide-large-min J]]
                              [--mums [--only many]] [--mums-large [--sweep]] [--kchain [--large-scan] [--python-jobs N]]

Workload: J jobs of 2 x L bases, L uniform in lmin .. lmax, 1 % substitutions.  The two sides run alternately, `reps` times each:
  loop   rv_reset, rv_add_sample / rv_add_sequence x 2, rv_construct, rv_align_builtin, rv_fetch_anchors, the text -- per job, straight at
         the C ABI (no Python object per job); with RV_LIB_DIR set this side runs on another build of the libraries (the parent commit's)
  many   reveal_amd.many: Batch.add x J, run, anchors (the C part), and align_many as a whole (with the Python result lists)
Prints medians, the loop's spread, the ratio and one JSON line.  --check compares the two sides' anchors job by job.
--seqs K: jobs of K sequences (K copies of one ancestor, 1 % substitutions each; lmax is cut so that every job stays within 2048 ranks).
--multi 0 / 1 sets RV_MANY_MULTI of the `many` side (jobs of 3 .. 16 sequences through the shared launches).  --multi ab: no loop; two batches,
switch off and on, run alternately in one process -- medians, both spreads, the ratio, and with --check the jobs that differ between the sides.
--large 0 / 1 / ab: the same for RV_MANY_LARGE (pair jobs above 2048 ranks through shared launches; choose --lmin / --lmax above 1023);
--large-multi 0 / 1 / ab: the same for RV_MANY_LARGE_MULTI (jobs of --seqs K >= 3 sequences above 2048 ranks; lmax is not cut then: choose
--lmin / --lmax so that K x (L + 1) lies above 2048).  The ab legs also print the levels and scanned ranks of a call (the run's statistics).
--large-max / --large-min set RV_MANY_LARGE_MAX / RV_MANY_LARGE_MIN of every batch (with --large-multi: RV_MANY_LARGE_MULTI_MIN too).
--wide 0 / 1 / ab: the same for RV_MANY_WIDE (jobs of --seqs K = 17 .. 64 sequences).  lmax is cut to 2048 ranks a job as with --multi; with
--no-cut it is not (choose --lmin / --lmax so that K x (L + 1) lies above 2048: the sample-major rounds of the wide jobs).  --wide-large-min
sets RV_MANY_WIDE_LARGE_MIN of every batch.  --sites: the K members of a job differ at one to three variant sites, each substituted in a
random subset of the members (the bubble of K haplotypes), not by 1 % substitutions per member -- among 32 or 64 members those leave almost
no window common to all, and a call anchors next to nothing.
--picker: the reference's default picker (rem.align's defaults: wpen 1, wscore 1, sumofpairs, trim, seedsize 10000, maxmums 10000) instead of the
built-in one, no loop through a handle; three batches run alternately in one process -- RV_MANY_CHAIN on (the leaf kernel with the picker's decision
as its pick stage), RV_MANY_CHAIN off (every job the ordinary way, the picker in host C++), and the built-in picker on the same jobs -- then
`rem.align` per job over the first --rem-jobs jobs (default 1000), once: the route to these anchors without align_many.  --check compares the two
picker sides job by job, and the jobs of the rem.align loop with it.
--picker --seqs K (K = 3 .. 16): the same for jobs of K sequences -- RV_MANY_CHAIN_MULTI on (the multi-sample leaf kernel with the picker as its pick
stage), off (the ordinary path), and the built-in picker with RV_MANY_MULTI on (k_leaf_multi on the same jobs).  With RV_LIB_DIR set to a build from
before the switch the first side is left out: the other two are that build's ordinary path and its k_leaf_multi, the baselines of the parent commit.
--chain-wide (with --seqs K, K = 17 .. 64; implies --picker; use --sites): the same for jobs of K sequences -- RV_MANY_CHAIN_WIDE on (the 64-sample form of
that kernel), off (the ordinary path), and the built-in picker with RV_MANY_WIDE on (k_leaf_multi<64> on the same jobs).  The chain side's
--picker --chain-large (pair jobs; choose --lmin / --lmax above 1023, e.g. 1100 / 9999): the same for pair jobs above 2048 ranks -- RV_MANY_CHAIN_LARGE on (the
level pipeline with the picker's decision made by k_pick_chain and k_leaf_chain), off (the ordinary path), and the built-in picker with RV_MANY_LARGE on (the
same rounds with the longest-match kernel).  --chain-large-min J sets RV_MANY_CHAIN_LARGE_MIN.  With RV_LIB_DIR set to a build from before the switch the
ordinary side alone is timed, on the same jobs: the yardstick.
--picker --chain-large-multi (with --seqs K, K = 3 .. 16; choose --lmin / --lmax so that the jobs lie above 2048 ranks, and --maxmums / --seedsize above their
ranks / sequences so that all are admitted): the same for jobs of K sequences above 2048 ranks -- RV_MANY_CHAIN_LARGE_MULTI on (the multi-sample level pipeline
with the picker's decision made by k_pick_multi_chain), off (the ordinary path), and the built-in picker with RV_MANY_LARGE_MULTI on (the same rounds with the
longest-match kernels).  --chain-large-multi-min J sets RV_MANY_CHAIN_LARGE_MULTI_MIN.
--chain-wide-large (with --seqs K, K = 17 .. 64; implies --picker and --no-cut; use --sites, --lmin / --lmax so that the jobs lie above 2048 ranks, and --maxmums /
--seedsize above their ranks / sequences): the same for jobs of K sequences above 2048 ranks -- RV_MANY_CHAIN_WIDE_LARGE on (the 64-sample form of
k_pick_multi_chain), off (the ordinary path), and the built-in picker with RV_MANY_WIDE on (the same rounds with the longest-match kernels).
--chain-wide-large-min J sets RV_MANY_CHAIN_WIDE_LARGE_MIN.  The chain side also prints the jobs it gave back by the bits of their flag words (Batch.flagged).
The chain side's info["ordinary"] is the number of jobs the kernel flagged.  --save-digests FILE writes a digest per job of the picker side's anchors (the chain side, or
the ordinary side where the build has none); --compare-digests FILE counts the jobs whose digest differs from that file's: two builds run in a process
each, and this is how their results are compared.
--mums (with --seqs K, 2 .. 64): the match lists instead of alignments -- Batch.add x J, scan (kind auto), matches -- on three legs run alternately in one
process: the shared path, the same call with RV_MANY_SCAN_ORDINARY, and the loop through one reused handle (rv_reset, add, rv_construct, rv_getmums /
rv_getmultimums, fetch: calls the commit before mums_many has too).  Medians, spreads, jobs per second, the gate (the shared median below the loop's by
more than both spreads), then both sides at 1, 4, 16, 64 and 256 jobs.  --check compares the legs job by job.  Exit status 1 when the gate is missed.
--mums-large (with --seqs K, 2 .. 64; implies --no-cut; choose --lmin / --lmax so that K x (L + 1) lies above 2048): the same for jobs above 2048 ranks -- the shared
path with RV_MANY_SCAN_LARGE on (RV_MANY_SCAN_LARGE_MIN 1), the same call with the switch off (every such job the ordinary way inside the call), and the loop through one
reused handle, alternately in one process, every leg ending with its results on the host.  The gate: the shared median below the switch-off leg's by more than the larger
of the two spreads.  --sweep: then shared against switch-off at 1, 2, 4, 8 and 16 jobs a call (the evidence for the default of RV_MANY_SCAN_LARGE_MIN).
--kchain-big [--kb-ks 2,3,8] [--kb-logm 8,17] [--kb-host-once S] [--kb-host-skip S] [--kb-budget S] [--kb-recurse L] [--kb-only lists|many|recurse]: the chaining
programme in device memory (rv_kchain_big.hip) against RV_MANY_KCHAIN_BIG = 0 (every list on the host: the parent commit's behaviour), alternately in one process, five
repetitions after a full-size warm-up per leg, medians and spreads: abstract lists of m = 2^8 .. 2^17 points through rv_many_kchain_lists with RV_KCHAIN_BIG_MIN = 1 (a
host leg expected above --kb-host-once seconds runs once, without a warm-up; one expected above --kb-host-skip seconds is left out; both are said), 16 lists of 4096
points in one call, and chain_recurse on two synthetic genomes of --kb-recurse bases (1 % variants, a fifth of them indels) at the defaults.  The gate per workload: the
big leg's median below the host leg's by more than both spreads."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reveal_amd import _lib, reveallib      # noqa: E402


def workload(jobs, lmin, lmax, seed=1, seqs=2, cut=True, sites=False):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", np.uint8)
    out = []
    if seqs > 2 and cut:
        lmax = min(lmax, (2048 - seqs) // seqs)
        lmin = min(lmin, lmax)
    for _ in range(jobs):
        L = int(rng.integers(lmin, lmax + 1))
        a = rng.integers(0, 4, L)
        if seqs > 2 and sites:      # one to three variant sites, each substituted in a random non-empty proper subset of the members
            fam = np.tile(a, (seqs, 1))
            for p in rng.choice(L, size=min(L, int(rng.integers(1, 4))), replace=False):
                who = rng.choice(seqs, size=int(rng.integers(1, seqs)), replace=False)
                fam[who, p] = (a[p] + int(rng.integers(1, 4))) % 4
            out.append([lut[r].tobytes() for r in fam])
            continue
        if seqs > 2:
            job = []
            for _ in range(seqs):
                b = a.copy()
                hit = rng.random(L) < 0.01
                b[hit] = (b[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
                job.append(lut[b].tobytes())
            out.append(job)
            continue
        b = a.copy()
        hit = rng.random(L) < 0.01
        b[hit] = (b[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        out.append([lut[a].tobytes(), lut[b].tobytes()])
    return out


def run_loop(idx, jobs, minl):
    """the jobs one after the other through one handle; -> per job (l[], pos[] of all members, off[])"""
    dll, h = idx._dll, idx._h
    st = _lib.RvAlignStats()
    mem = ctypes.c_int64(0)
    res = []
    for job in jobs:
        ok = dll.rv_reset(h) == 0
        for s in job:
            ok = ok and dll.rv_add_sample(h) == 0 and dll.rv_add_sequence(h, s, len(s), None, None) == 0
        ok = ok and dll.rv_construct(h, 0, None, None, 0) == 0 and dll.rv_align_builtin(h, minl, 2, ctypes.byref(st)) == 0
        if not ok:
            raise RuntimeError(idx._lib.err())
        na = dll.rv_anchor_count(h, ctypes.byref(mem))
        l = np.empty(max(na, 1), np.uint32); off = np.empty(na + 1, np.int64); pos = np.empty(max(mem.value, 1), np.int64)
        off[0] = 0
        n = sum(len(s) for s in job) + len(job)
        T = ctypes.create_string_buffer(n)
        if dll.rv_fetch_anchors(h, l.ctypes.data, off.ctypes.data, pos.ctypes.data) != 0 or dll.rv_get_array(h, _lib.RV_T, T, n) != n:
            raise RuntimeError(idx._lib.err())
        res.append((l[:na], pos[:mem.value], off))
    return res


def run_many_c(batch, jobs, minl):
    batch.clear()
    for j in jobs:
        batch.add(j)
    batch.last_stats = batch.run(minl, 2)
    return batch.anchors()


def as_lists(first, l, off, pos):
    """Batch.anchors() -> per job sorted [(l, members)]"""
    l, off, pos, first = l.tolist(), off.tolist(), pos.tolist(), first.tolist()
    return [sorted((l[k], tuple(pos[off[k]:off[k + 1]])) for k in range(first[j], first[j + 1])) for j in range(len(first) - 1)]


def more_options(a, b):
    if a.large_max is not None:
        b.option("RV_MANY_LARGE_MAX", a.large_max)
    if a.wide_large_min is not None:
        b.option("RV_MANY_WIDE_LARGE_MIN", a.wide_large_min)
    if a.large_min is not None:
        b.option("RV_MANY_LARGE_MIN", a.large_min)
        if a.large_multi is not None:
            from reveal_amd import many
            try:
                b.option("RV_MANY_LARGE_MULTI_MIN", a.large_min)
            except many.error:      # (RV_LIB_DIR: a build from before the switch has no such jobs to count)
                if a.large_multi != "0":
                    raise


def main_ab(a, jobs, bases, switch="RV_MANY_MULTI"):
    """`switch` (RV_MANY_MULTI, RV_MANY_LARGE, RV_MANY_LARGE_MULTI or RV_MANY_WIDE) off against on: two batches, alternately"""
    from reveal_amd import many
    sides = {}
    for name, v in (("off", 0), ("on", 1)):
        b = many.Batch(False)
        if switch != "RV_MANY_MULTI" and a.multi in ("0", "1"):
            b.option("RV_MANY_MULTI", int(a.multi))
        if switch != "RV_MANY_LARGE" and a.large in ("0", "1"):
            b.option("RV_MANY_LARGE", int(a.large))
        if switch != "RV_MANY_LARGE_MULTI" and a.large_multi in ("0", "1"):
            b.option("RV_MANY_LARGE_MULTI", int(a.large_multi))
        if switch != "RV_MANY_WIDE" and a.wide in ("0", "1"):
            b.option("RV_MANY_WIDE", int(a.wide))
        more_options(a, b)
        b.option(switch, v)
        if a.wave_max is not None:
            b.option("RV_MANY_WAVE_MAX", a.wave_max)
        run_many_c(b, jobs[:64], a.minlength)
        sides[name] = dict(batch=b, t=[], res=None)
    for rep in range(a.reps):
        for name in ("off", "on"):
            s = sides[name]
            t = time.perf_counter(); s["res"] = run_many_c(s["batch"], jobs, a.minlength); s["t"].append(time.perf_counter() - t)
    out = dict(jobs=a.jobs, seqs=a.seqs, lmin=a.lmin, lmax=a.lmax, bases=bases, minlength=a.minlength, reps=a.reps, switch=switch)
    for name in ("off", "on"):
        t = sides[name]["t"]
        out[name + "_s"] = t; out[name + "_median_s"] = statistics.median(t); out[name + "_spread_s"] = max(t) - min(t)
        out[name + "_info"] = sides[name]["batch"].info()
        st = sides[name]["batch"].last_stats
        out[name + "_levels"] = int(st["levels"]); out[name + "_scanned_ranks"] = int(st["scanned_ranks"])
        print("%-3s   : runs %s s; median %.4f s, spread (max - min) %.4f s, %.0f jobs/s; info %r; levels %d, scanned ranks %d"
              % (name, " ".join("%.4f" % x for x in t), out[name + "_median_s"], out[name + "_spread_s"], a.jobs / out[name + "_median_s"], out[name + "_info"],
                 out[name + "_levels"], out[name + "_scanned_ranks"]))
    out["ratio"] = out["off_median_s"] / out["on_median_s"]
    out["gain_s"] = out["off_median_s"] - out["on_median_s"]
    print("ratio : %.1f x  (gain %.4f s against the off side's spread of %.4f s)" % (out["ratio"], out["gain_s"], out["off_spread_s"]))
    if a.check:
        x, y = as_lists(*sides["off"]["res"]), as_lists(*sides["on"]["res"])
        out["check_bad_jobs"] = sum(1 for p, q in zip(x, y) if p != q)
        out["anchors"] = sum(len(p) for p in y)
        print("check : %d of %d jobs differ between the two sides (%d anchors)" % (out["check_bad_jobs"], a.jobs, out["anchors"]))
    print(json.dumps(out))
    return 1 if out.get("check_bad_jobs") else 0


def run_scan_loop(idx, jobs, minl, minn=2):
    """leg (c) of --mums: the jobs one after the other through one handle, straight at the C ABI -- rv_reset, add, rv_construct, rv_getmums (two
    sequences) or rv_getmultimums (more), and the fetch; -> per job (l, n, so, pos) with getmums' records as (0, a), (sample of b, b)"""
    dll, h = idx._dll, idx._h
    mem = ctypes.c_int64(0)
    res = []
    for job in jobs:
        ok = dll.rv_reset(h) == 0
        for s in job:
            ok = ok and dll.rv_add_sample(h) == 0 and dll.rv_add_sequence(h, s, len(s), None, None) == 0
        ok = ok and dll.rv_construct(h, 0, None, None, 0) == 0
        if not ok:
            raise RuntimeError(idx._lib.err())
        if len(job) == 2:
            nm = dll.rv_getmums(h, minl)
            if nm < 0:
                raise RuntimeError(idx._lib.err())
            l = np.empty(max(nm, 1), np.uint32); x = np.empty(max(nm, 1), np.int64); y = np.empty(max(nm, 1), np.int64)
            if dll.rv_fetch_mums(h, l.ctypes.data, x.ctypes.data, y.ctypes.data, nm) != 0:
                raise RuntimeError(idx._lib.err())
            pos = np.stack([x[:nm], y[:nm]], 1).reshape(-1)
            so = np.tile(np.array([0, 1], np.uint16), nm)
            res.append((l[:nm], np.full(nm, 2, np.int32), so, pos))
        else:
            nm = dll.rv_getmultimums(h, minl, minn, 0, ctypes.byref(mem))
            if nm < 0:
                raise RuntimeError(idx._lib.err())
            l = np.empty(max(nm, 1), np.uint32); n = np.empty(max(nm, 1), np.int32); off = np.empty(nm + 1, np.int64)
            so = np.empty(max(mem.value, 1), np.uint16); pos = np.empty(max(mem.value, 1), np.int64)
            if dll.rv_fetch_multi(h, l.ctypes.data, n.ctypes.data, off.ctypes.data, so.ctypes.data, pos.ctypes.data) != 0:
                raise RuntimeError(idx._lib.err())
            res.append((l[:nm], n[:nm], so[:mem.value], pos[:mem.value]))
    return res


def run_scan_c(batch, jobs, minl, minn=2):
    batch.clear()
    for j in jobs:
        batch.add(j)
    batch.scan(minl, minn, "auto")
    return batch.matches()


def main_mums(a, jobs, bases):
    """--mums: the match lists of every job (many.mums_many's C part: Batch.add x J, scan, matches) -- the shared path, the same call with
    RV_MANY_SCAN_ORDINARY, and the loop through one reused handle -- alternately in one process; then the smallest job count at which the
    shared path beats the loop, out of 1, 4, 16, 64, 256.  Every leg ends with its results on the host."""
    from reveal_amd import many
    idx = reveallib.index()
    shared, ordinary = many.Batch(False), many.Batch(False)
    ordinary.option("RV_MANY_SCAN_ORDINARY", 1)
    if a.wave_max is not None:
        shared.option("RV_MANY_WAVE_MAX", a.wave_max)
    legs = (("shared", lambda js: run_scan_c(shared, js, a.minlength)), ("ordinary", lambda js: run_scan_c(ordinary, js, a.minlength)),
            ("loop", lambda js: run_scan_loop(idx, js, a.minlength)))
    if a.only == "many":      # the shared leg alone (under a profiler: the kernels of the scan and nothing else)
        ts = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter(); run_scan_c(shared, jobs, a.minlength); ts.append(time.perf_counter() - t0)
        print("shared  : runs %s s (the first one cold); %r" % (" ".join("%.4f" % x for x in ts), shared.info()))
        return 0
    for _, f in legs:
        f(jobs[:64])      # (first use: allocations, code objects)
    t = {name: [] for name, _ in legs}
    res = {}
    for rep in range(a.reps):
        for name, f in legs:
            t0 = time.perf_counter(); res[name] = f(jobs); t[name].append(time.perf_counter() - t0)
    out = dict(mode="mums", jobs=a.jobs, seqs=a.seqs, lmin=a.lmin, lmax=a.lmax, bases=bases, minlength=a.minlength, reps=a.reps, lib_dir=os.environ.get("RV_LIB_DIR", ""))
    for name, _ in legs:
        out[name + "_s"] = t[name]; out[name + "_median_s"] = statistics.median(t[name]); out[name + "_spread_s"] = max(t[name]) - min(t[name])
        print("%-8s: runs %s s; median %.4f s, spread (max - min) %.4f s, %.0f jobs/s"
              % (name, " ".join("%.4f" % x for x in t[name]), out[name + "_median_s"], out[name + "_spread_s"], a.jobs / out[name + "_median_s"]))
    out["shared_info"] = shared.info(); out["ordinary_info"] = ordinary.info()
    out["matches"] = int(len(res["shared"][1])); out["members"] = int(len(res["shared"][5]))
    out["ratio_loop"] = out["loop_median_s"] / out["shared_median_s"]; out["ratio_ordinary"] = out["ordinary_median_s"] / out["shared_median_s"]
    out["gate"] = bool(out["loop_median_s"] - out["shared_median_s"] > out["loop_spread_s"] + out["shared_spread_s"])
    print("shared against the loop: %.1f x (gain %.4f s against spreads of %.4f + %.4f s: gate %s); against the ordinary leg: %.1f x; %d matches, %d members; %r"
          % (out["ratio_loop"], out["loop_median_s"] - out["shared_median_s"], out["loop_spread_s"], out["shared_spread_s"], "met" if out["gate"] else "MISSED",
             out["ratio_ordinary"], out["matches"], out["members"], out["shared_info"]))
    if a.check:
        first, l, n, off, so, pos = res["shared"]
        same = all(np.array_equal(x, y) for x, y in zip(res["shared"], res["ordinary"]))
        bad = 0
        for j, (ll, ln, lso, lpos) in enumerate(res["loop"]):
            lo, hi = int(first[j]), int(first[j + 1])
            bad += not (np.array_equal(l[lo:hi], ll) and np.array_equal(n[lo:hi], ln) and np.array_equal(so[off[lo]:off[hi]], lso) and np.array_equal(pos[off[lo]:off[hi]], lpos))
        out["check_ordinary_same"] = bool(same); out["check_bad_jobs"] = int(bad) + (0 if same else 1)
        print("check : shared and ordinary arrays %s; %d of %d jobs differ between the shared leg and the loop" % ("identical" if same else "DIFFER", bad, a.jobs))
    small = {}
    for J in (1, 4, 16, 64, 256):
        if J > len(jobs):
            break
        ts, tl = [], []
        for rep in range(max(a.reps, 5)):
            t0 = time.perf_counter(); run_scan_c(shared, jobs[:J], a.minlength); ts.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); run_scan_loop(idx, jobs[:J], a.minlength); tl.append(time.perf_counter() - t0)
        small[J] = dict(shared_median_s=statistics.median(ts), shared_spread_s=max(ts) - min(ts), loop_median_s=statistics.median(tl), loop_spread_s=max(tl) - min(tl))
        print("%4d jobs: shared median %.6f s (spread %.6f), loop median %.6f s (spread %.6f)" % (J, small[J]["shared_median_s"], small[J]["shared_spread_s"],
                                                                                                small[J]["loop_median_s"], small[J]["loop_spread_s"]))
    out["small"] = small
    wins = [J for J, v in small.items() if v["shared_median_s"] < v["loop_median_s"]]
    out["smallest_winning_jobs"] = min(wins) if wins else None
    print("smallest job count at which the shared path beats the loop: %s" % out["smallest_winning_jobs"])
    print(json.dumps(out))
    return 1 if out.get("check_bad_jobs") or not out["gate"] else 0


def main_mums_large(a, jobs, bases):
    """--mums-large: the match lists of jobs above 2048 ranks -- RV_MANY_SCAN_LARGE on, off, and the loop through one reused handle -- alternately in one
    process; --sweep: on against off at 1 .. 16 jobs a call.  Every leg ends with its results on the host."""
    from reveal_amd import many
    idx = reveallib.index()
    shared, off = many.Batch(False), many.Batch(False)
    shared.option("RV_MANY_SCAN_LARGE", 1)
    shared.option("RV_MANY_SCAN_LARGE_MIN", 1)
    off.option("RV_MANY_SCAN_LARGE", 0)
    legs = (("shared", lambda js: run_scan_c(shared, js, a.minlength)), ("off", lambda js: run_scan_c(off, js, a.minlength)),
            ("loop", lambda js: run_scan_loop(idx, js, a.minlength)))
    for _, f in legs:
        f(jobs[:16])      # (first use: allocations, code objects)
    t = {name: [] for name, _ in legs}
    res = {}
    for rep in range(a.reps):
        for name, f in legs:
            t0 = time.perf_counter(); res[name] = f(jobs); t[name].append(time.perf_counter() - t0)
    ranks = [sum(len(s) for s in j) + len(j) for j in jobs]
    out = dict(mode="mums-large", jobs=a.jobs, seqs=a.seqs, lmin=a.lmin, lmax=a.lmax, bases=bases, ranks_min=min(ranks), ranks_max=max(ranks), minlength=a.minlength, reps=a.reps)
    for name, _ in legs:
        out[name + "_s"] = t[name]; out[name + "_median_s"] = statistics.median(t[name]); out[name + "_spread_s"] = max(t[name]) - min(t[name])
        print("%-8s: runs %s s; median %.4f s, spread (max - min) %.4f s, %.0f jobs/s"
              % (name, " ".join("%.4f" % x for x in t[name]), out[name + "_median_s"], out[name + "_spread_s"], a.jobs / out[name + "_median_s"]))
    out["shared_info"] = shared.info(); out["off_info"] = off.info()
    out["matches"] = int(len(res["shared"][1])); out["members"] = int(len(res["shared"][5]))
    out["ratio_off"] = out["off_median_s"] / out["shared_median_s"]; out["ratio_loop"] = out["loop_median_s"] / out["shared_median_s"]
    out["gate"] = bool(out["off_median_s"] - out["shared_median_s"] > max(out["off_spread_s"], out["shared_spread_s"]))
    print("shared against the switch-off leg: %.1f x (gain %.4f s against spreads of %.4f and %.4f s: gate %s); against the loop: %.1f x; %d .. %d ranks a job; %d matches, %d members; shared %r; off %r"
          % (out["ratio_off"], out["off_median_s"] - out["shared_median_s"], out["off_spread_s"], out["shared_spread_s"], "met" if out["gate"] else "MISSED",
             out["ratio_loop"], out["ranks_min"], out["ranks_max"], out["matches"], out["members"], out["shared_info"], out["off_info"]))
    if a.check:
        first, l, n, off_, so, pos = res["shared"]
        same = all(np.array_equal(x, y) for x, y in zip(res["shared"], res["off"]))
        bad = 0
        for j, (ll, ln, lso, lpos) in enumerate(res["loop"]):
            lo, hi = int(first[j]), int(first[j + 1])
            bad += not (np.array_equal(l[lo:hi], ll) and np.array_equal(n[lo:hi], ln) and np.array_equal(so[off_[lo]:off_[hi]], lso) and np.array_equal(pos[off_[lo]:off_[hi]], lpos))
        out["check_off_same"] = bool(same); out["check_bad_jobs"] = int(bad) + (0 if same else 1)
        print("check : shared and switch-off arrays %s; %d of %d jobs differ between the shared leg and the loop" % ("identical" if same else "DIFFER", bad, a.jobs))
    if a.sweep:
        small = {}
        for J in (1, 2, 4, 8, 16):
            if J > len(jobs):
                break
            ts, to = [], []
            for rep in range(max(a.reps, 9)):
                js = jobs[rep * J:(rep + 1) * J] if (rep + 1) * J <= len(jobs) else jobs[:J]      # (other jobs every time: sizes vary 1 : 14)
                t0 = time.perf_counter(); run_scan_c(shared, js, a.minlength); ts.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); run_scan_c(off, js, a.minlength); to.append(time.perf_counter() - t0)
            small[J] = dict(shared_median_s=statistics.median(ts), shared_spread_s=max(ts) - min(ts), off_median_s=statistics.median(to), off_spread_s=max(to) - min(to))
            print("%4d jobs: shared median %.6f s (spread %.6f), switch off median %.6f s (spread %.6f)" % (J, small[J]["shared_median_s"], small[J]["shared_spread_s"],
                                                                                                          small[J]["off_median_s"], small[J]["off_spread_s"]))
        out["sweep"] = small
        ok = [J for J in small if all(small[K]["shared_median_s"] <= small[K]["off_median_s"] for K in small if K >= J)]
        out["smallest_not_slower_jobs"] = min(ok) if ok else None
        print("smallest job count from which the shared path is not slower: %s" % out["smallest_not_slower_jobs"])
    print(json.dumps(out))
    return 1 if out.get("check_bad_jobs") or not out["gate"] else 0


def run_kchain_c(batch, jobs, minl):
    batch.clear()
    for j in jobs:
        batch.add(j)
    batch.kchain(minl)
    return batch.chains()


def main_kchain(a, jobs, bases):
    """--kchain: the collinear chain of every job (kchain.kchain_many's C part: Batch.add x J, kchain, chains) -- chained on the device, the same call with
    RV_MANY_KCHAIN_HOST, and the means of a build without it: the scan of every job (kind multimums) with the lists taken apart on the host, then
    kchain.kchain_python per job -- alternately in one process.  Every leg ends with its paths on the host.  --python-jobs N: kchain_python on the first N
    jobs only (the scan still on all of them), its share scaled to all jobs and said so.  The D2H bytes are computed from the sizes of what each call
    copies back (records 16 bytes, members 6; nodes 12, their positions 4, 20 bytes a job), not measured."""
    from reveal_amd import kchain, many
    dev, host, scan = many.Batch(False), many.Batch(False), many.Batch(False)
    host.option("RV_MANY_KCHAIN_HOST", 1)
    for b in (dev, host, scan):
        if a.large_scan:
            b.option("RV_MANY_SCAN_LARGE", 1)
    npy = min(a.python_jobs if a.python_jobs is not None else len(jobs), len(jobs))

    def run_python(js, count):
        scan.clear()
        for j in js:
            scan.add(j)
        scan.scan(a.minlength, 2, "multimums")
        t1 = time.perf_counter()
        m = many.Matches(scan.matches(), [False] * len(js))
        paths = [kchain.kchain_python(m[j], [len(s) for s in js[j]]) for j in range(min(count, len(js)))]
        return paths, time.perf_counter() - t1
    legs = (("device", lambda js: run_kchain_c(dev, js, a.minlength)), ("host", lambda js: run_kchain_c(host, js, a.minlength)))
    for _, f in legs:
        f(jobs)      # (first use at full size: allocations, code objects)
    run_python(jobs, 8)
    t = {"device": [], "host": [], "python": []}
    res = {}
    for rep in range(a.reps):
        for name, f in legs:
            t0 = time.perf_counter(); res[name] = f(jobs); t[name].append(time.perf_counter() - t0)
        t0 = time.perf_counter(); res["python"], tpy = run_python(jobs, npy); whole = time.perf_counter() - t0
        t["python"].append(whole - tpy + tpy * len(jobs) / max(npy, 1))
    out = dict(mode="kchain", jobs=a.jobs, seqs=a.seqs, lmin=a.lmin, lmax=a.lmax, bases=bases, minlength=a.minlength, reps=a.reps, large=bool(a.large_scan), python_jobs=npy)
    for name in t:
        out[name + "_s"] = t[name]; out[name + "_median_s"] = statistics.median(t[name]); out[name + "_spread_s"] = max(t[name]) - min(t[name])
        print("%-8s: runs %s s; median %.4f s, spread (max - min) %.4f s, %.0f jobs/s%s"
              % (name, " ".join("%.4f" % x for x in t[name]), out[name + "_median_s"], out[name + "_spread_s"], a.jobs / out[name + "_median_s"],
                 "" if name != "python" or npy == len(jobs) else " (kchain_python on %d jobs, scaled)" % npy))
    first, l, score, pos, end = res["device"]
    out["device_info"] = dev.info(); out["host_info"] = host.info(); out["flagged"] = dev.flagged().get(kchain.KCHAIN_FLAG, 0)
    out["nodes"] = int(len(l)); out["positions"] = int(len(pos))
    mfirst, ml, mn, moff, mso, mpos = scan.matches()
    out["records"] = int(len(ml)); out["members"] = int(len(mpos))
    out["d2h_scan_bytes"] = out["records"] * 16 + out["members"] * 6 + (len(jobs) + 1) * 8
    out["d2h_kchain_bytes"] = out["nodes"] * 12 + out["positions"] * 4 + len(jobs) * 20 + 2 * (len(jobs) + 1) * 8
    gain = out["host_median_s"] - out["device_median_s"]
    out["gate"] = bool(gain > max(out["host_spread_s"], out["device_spread_s"]))
    same = all(np.array_equal(x, y) for x, y in zip(res["device"], res["host"]))
    bad = 0
    k_of = [len(j) for j in jobs]
    ch = kchain.Chains(res["device"], k_of)
    for j, (path, e) in enumerate(res["python"]):
        bad += not (ch[j] == path and int(end[j]) == e)
    out["check_host_same"] = bool(same); out["check_bad_jobs"] = int(bad) + (0 if same else 1)
    print("device against RV_MANY_KCHAIN_HOST: %.2f x (gain %.4f s against spreads of %.4f and %.4f s: gate %s); against scan + kchain_python: %.1f x; %d nodes of %d records;"
          " D2H %d bytes against the scan's %d; %d jobs flagged; device %r" % (out["host_median_s"] / out["device_median_s"], gain, out["host_spread_s"], out["device_spread_s"],
                                                                             "met" if out["gate"] else "MISSED", out["python_median_s"] / out["device_median_s"], out["nodes"], out["records"],
                                                                             out["d2h_kchain_bytes"], out["d2h_scan_bytes"], out["flagged"], out["device_info"]))
    print("check : device and host arrays %s; %d of %d jobs differ between the device leg and kchain_python" % ("identical" if same else "DIFFER", bad, npy))
    print(json.dumps(out))
    return 1 if out["check_bad_jobs"] or not out["gate"] else 0


def kb_lists(k, m, nlists, seed):
    """nlists abstract lists of m points in k sequences as the arrays of rv_many_kchain_lists: distinct coordinates in every dimension, a tenth of the
    points off the backbone in each dimension behind the first, lengths 1 .. 40, records in random order"""
    rng = np.random.Generator(np.random.PCG64(seed))
    span = 40 * m + 200
    ls, ns, sos, poss, lens = [], [], [], [], []
    for _ in range(nlists):
        ln = [span + 40 + int(rng.integers(0, 31)) for _ in range(k)]
        begin = np.concatenate([[0], np.cumsum(np.array(ln[:-1], np.int64) + 1)])
        cols = np.stack([np.sort(rng.choice(span, size=m, replace=False)) for _ in range(k)], axis=1).astype(np.int64)
        for d in range(1, k):
            a_, b_ = rng.integers(0, m, size=m // 10), rng.integers(0, m, size=m // 10)
            for x, y in zip(a_, b_):
                cols[x, d], cols[y, d] = cols[y, d], cols[x, d]
        cols = cols[rng.permutation(m)]
        ls.append(rng.integers(1, 41, size=m).astype(np.uint32)); ns.append(np.full(m, k, np.int32))
        sos.append(np.tile(np.arange(k, dtype=np.uint16), m)); poss.append((cols + begin[None, :]).reshape(-1)); lens += ln
    tot = m * nlists
    return (np.full(nlists, k, np.int32), np.full(nlists, m, np.int64), np.concatenate(ls), np.concatenate(ns), np.arange(tot + 1, dtype=np.int64) * k,
            np.concatenate(sos), np.concatenate(poss), np.array(lens, np.int64))


def kb_call(b, arrs, nlists):
    ks, nrec, l, n, off, so, pos, ln = arrs
    if b._dll.rv_many_kchain_lists(b._m, nlists, ks.ctypes.data, nrec.ctypes.data, l.ctypes.data, n.ctypes.data, off.ctypes.data, so.ctypes.data, pos.ctypes.data,
                                   ln.ctypes.data, 0, 1, 1, 0) != 0:
        b._fail()
    return b.chains(nlists)


def kb_legs(name, big_f, host_f, reps, host_mode, out):
    """the two legs alternately; host_mode: "reps", "once" (no warm-up, one run) or "skip" """
    t = {"big": [], "host": []}
    res = {}
    big_f()
    if host_mode == "reps":
        host_f()
    for rep in range(reps):
        t0 = time.perf_counter(); res["big"] = big_f(); t["big"].append(time.perf_counter() - t0)
        if host_mode == "reps" or (host_mode == "once" and rep == 0):
            t0 = time.perf_counter(); res["host"] = host_f(); t["host"].append(time.perf_counter() - t0)
    r = dict(workload=name, host_mode=host_mode, big_s=t["big"], host_s=t["host"], big_median_s=statistics.median(t["big"]), big_spread_s=max(t["big"]) - min(t["big"]))
    line = "%-34s big: median %.5f s, spread %.5f s" % (name, r["big_median_s"], r["big_spread_s"])
    if t["host"]:
        r["host_median_s"] = statistics.median(t["host"]); r["host_spread_s"] = max(t["host"]) - min(t["host"])
        r["same"] = bool(all(np.array_equal(x, y) for x, y in zip(res["big"], res["host"])))
        r["gate"] = bool(r["host_median_s"] - r["big_median_s"] > max(r["host_spread_s"], r["big_spread_s"])) if host_mode == "reps" else None
        line += "; host: median %.5f s, spread %.5f s%s; %.2f x; gate %s; results %s" % (
            r["host_median_s"], r["host_spread_s"], " (ONE run, no warm-up)" if host_mode == "once" else "", r["host_median_s"] / r["big_median_s"],
            "not judged" if r["gate"] is None else "met" if r["gate"] else "MISSED", "identical" if r["same"] else "DIFFER")
    else:
        line += "; host leg left out (expected above the limit)"
    print(line, flush=True)
    out.append(r)
    return r


def main_kchain_big(a):
    from reveal_amd import kchain, many, synth
    t_start = time.perf_counter()
    big, host = many.Batch(False), many.Batch(False)
    big.option("RV_KCHAIN_BIG_MIN", 1)
    host.option("RV_MANY_KCHAIN_BIG", 0)
    out = []
    lo, hi = (int(x) for x in a.kb_logm.split(","))
    if a.kb_only in (None, "lists"):
        for k in (int(x) for x in a.kb_ks.split(",")):
            expect = 0.0
            for lg in range(lo, hi + 1):
                if time.perf_counter() - t_start > a.kb_budget:
                    print("k = %d: stopped in front of m = 2^%d (the time budget of this run)" % (k, lg), flush=True)
                    break
                m = 1 << lg
                arrs = kb_lists(k, m, 1, 100 * k + lg)
                mode = "skip" if expect > a.kb_host_skip else "once" if expect > a.kb_host_once else "reps"
                r = kb_legs("lists k=%d m=2^%d" % (k, lg), lambda: kb_call(big, arrs, 1), lambda: kb_call(host, arrs, 1), a.reps, mode, out)
                r["launches"] = big.kchain_big()[1]; r["big_lists"] = big.kchain_big()[0]
                expect = 4 * r.get("host_median_s", expect)
    if a.kb_only in (None, "many"):
        arrs = kb_lists(2, 4096, 16, 7)
        r = kb_legs("16 lists k=2 m=4096, one call", lambda: kb_call(big, arrs, 16), lambda: kb_call(host, arrs, 16), a.reps, "reps", out)
        r["launches"] = big.kchain_big()[1]; r["big_lists"] = big.kchain_big()[0]
    if a.kb_only in (None, "recurse") and a.kb_recurse > 0:
        seqs = [g.decode() for g in synth.genomes(a.kb_recurse, 2, snp=0.01, indelfrac=0.2)]
        dflt, off = many.Batch(False), many.Batch(False)
        off.option("RV_MANY_KCHAIN_BIG", 0)
        infos = {}

        def rec(b, key):
            an, infos[key] = kchain.chain_recurse(seqs, batch=b, toupper=False)
            return (np.array([x[0] for x in an]), np.array([p for x in an for _, p in x[1]]), np.array([x[2] for x in an]))
        r = kb_legs("chain_recurse 2 x %d bases" % a.kb_recurse, lambda: rec(dflt, "big"), lambda: rec(off, "host"), a.reps, "reps", out)
        r["levels"] = len(infos["big"]); r["top_big"] = infos["big"][0]["big"]; r["top_launches"] = infos["big"][0]["big_launches"]; r["top_info"] = infos["big"][0]
        print("chain_recurse: %d levels; top level %r" % (r["levels"], infos["big"][0]), flush=True)
    print(json.dumps(dict(mode="kchain-big", reps=a.reps, lib_dir=os.environ.get("RV_LIB_DIR"), results=out)))
    return 0


def main_picker(a, jobs, bases):
    """the reference's default picker: RV_MANY_CHAIN on / off, the built-in picker beside them, rem.align per job"""
    from reveal_amd import many, rem, schemes
    args = schemes.PickerArgs(maxmums=a.maxmums, seedsize=a.seedsize)      # (10 000 / 10 000: rem.align's defaults)
    sides = {}
    switch = "RV_MANY_CHAIN" if a.seqs == 2 else ("RV_MANY_CHAIN_MULTI" if a.seqs <= 16 else "RV_MANY_CHAIN_WIDE")
    if a.chain_large:
        switch = "RV_MANY_CHAIN_LARGE"
    if a.chain_large_multi:
        switch = "RV_MANY_CHAIN_LARGE_MULTI"
    if a.chain_wide_large:
        switch = "RV_MANY_CHAIN_WIDE_LARGE"
    for name, pk, chain in (("chain", args, 1), ("ordinary", args, 0), ("builtin", None, 0)):
        b = many.Batch(False)
        b.set_picker(pk)
        try:
            b.option(switch, chain)
        except many.error:      # (RV_LIB_DIR: a build from before the switch -- off is all it knows)
            if chain:
                print("%s is not known to this build: no chain side" % switch)
                continue
        if a.seqs > 2 and pk is None:
            b.option("RV_MANY_MULTI" if a.seqs <= 16 else "RV_MANY_WIDE", 1)
        if a.chain_large_multi and pk is None:
            b.option("RV_MANY_LARGE_MULTI", 1)
            b.option("RV_MANY_LARGE_MULTI_MIN", 1)
        if a.chain_large_multi and chain and a.chain_large_multi_min is not None:
            b.option("RV_MANY_CHAIN_LARGE_MULTI_MIN", a.chain_large_multi_min)
        if a.chain_wide_large and pk is None:
            b.option("RV_MANY_WIDE_LARGE_MIN", 1)
        if a.chain_wide_large and chain and a.chain_wide_large_min is not None:
            b.option("RV_MANY_CHAIN_WIDE_LARGE_MIN", a.chain_wide_large_min)
        if a.chain_large and pk is None:
            b.option("RV_MANY_LARGE", 1)
        if a.chain_large and chain and a.chain_large_min is not None:
            b.option("RV_MANY_CHAIN_LARGE_MIN", a.chain_large_min)
        if a.wave_max is not None:
            b.option("RV_MANY_WAVE_MAX", a.wave_max)
        run_many_c(b, jobs[:64], a.minlength)
        sides[name] = dict(batch=b, t=[], res=None)
    for rep in range(a.reps):
        for name, s in sides.items():
            t = time.perf_counter(); s["res"] = run_many_c(s["batch"], jobs, a.minlength); s["t"].append(time.perf_counter() - t)
    out = dict(jobs=a.jobs, seqs=a.seqs, lmin=a.lmin, lmax=a.lmax, bases=bases, minlength=a.minlength, reps=a.reps, picker="graphmumpicker", lib_dir=os.environ.get("RV_LIB_DIR", ""))
    for name, s in sides.items():
        t = s["t"]
        out[name + "_s"] = t; out[name + "_median_s"] = statistics.median(t); out[name + "_spread_s"] = max(t) - min(t); out[name + "_info"] = s["batch"].info()
        print("%-8s: runs %s s; median %.4f s, spread (max - min) %.4f s, %.0f jobs/s; info %r"
              % (name, " ".join("%.4f" % x for x in t), out[name + "_median_s"], out[name + "_spread_s"], a.jobs / out[name + "_median_s"], out[name + "_info"]))
    if a.save_digests or a.compare_digests:
        side = "chain" if "chain" in sides else "ordinary"
        dig = [hashlib.sha256(repr(x).encode()).hexdigest()[:12] for x in as_lists(*sides[side]["res"])]
        if a.save_digests:
            with open(a.save_digests, "w") as f:
                json.dump(dig, f)
        if a.compare_digests:
            with open(a.compare_digests) as f:
                other = json.load(f)
            out["digest_bad_jobs"] = sum(1 for p, q in zip(dig, other) if p != q) + abs(len(dig) - len(other))
            print("digests: %d of %d jobs of the %s side differ from %s" % (out["digest_bad_jobs"], a.jobs, side, a.compare_digests))
    nrem = min(a.rem_jobs, len(jobs))
    rem_res = []
    t = time.perf_counter()
    for job in jobs[:nrem]:
        rem_res.append(rem.align([("s%d" % k, s.decode()) for k, s in enumerate(job)], minlength=a.minlength, maxmums=a.maxmums, seedsize=a.seedsize))
    out["rem_jobs"] = nrem; out["rem_s"] = time.perf_counter() - t
    out["rem_per_job_s"] = out["rem_s"] / max(nrem, 1)
    print("rem.align per job: %d jobs in %.2f s, %.2f ms a job, %.0f jobs/s" % (nrem, out["rem_s"], 1e3 * out["rem_per_job_s"], nrem / out["rem_s"]))
    if "chain" not in sides:
        print(json.dumps(out))
        return 1 if out.get("digest_bad_jobs") else 0
    out["flagged"] = out["chain_info"]["ordinary"]
    if hasattr(sides["chain"]["batch"], "flagged"):
        out["flagged_by_bit"] = sides["chain"]["batch"].flagged()
        print("flagged: %d jobs of the chain side went back to the ordinary path; by bit of their flag words: %r" % (out["flagged"], out["flagged_by_bit"] or "none"))
    out["chain_vs_rem"] = out["rem_per_job_s"] / (out["chain_median_s"] / a.jobs)
    out["ordinary_vs_chain"] = out["ordinary_median_s"] / out["chain_median_s"]
    out["chain_vs_builtin"] = out["chain_median_s"] / out["builtin_median_s"]
    print("ratio : rem.align per job / chain = %.0f x; ordinary / chain = %.1f x; chain / built-in picker = %.2f x (a job: %.2f against %.2f us)"
          % (out["chain_vs_rem"], out["ordinary_vs_chain"], out["chain_vs_builtin"], 1e6 * out["chain_median_s"] / a.jobs, 1e6 * out["builtin_median_s"] / a.jobs))
    if a.check:
        x, y = as_lists(*sides["chain"]["res"]), as_lists(*sides["ordinary"]["res"])
        out["check_bad_jobs"] = sum(1 for p, q in zip(x, y) if p != q)
        out["anchors"] = sum(len(p) for p in x)
        out["differ_from_builtin"] = sum(1 for p, q in zip(x, as_lists(*sides["builtin"]["res"])) if p != q)
        # (the final text of rem.align's index says which positions its anchors cover)
        bad = 0
        for j, (G, idx) in enumerate(rem_res):
            T = bytearray(b"$".join(jobs[j]) + b"$")
            for l, pos in x[j]:
                for p in pos:
                    T[p:p + l] = T[p:p + l].lower()
            bad += bytes(T) != idx.T.encode("latin-1")
        out["check_bad_rem_jobs"] = bad
        print("check : %d of %d jobs differ between chain and ordinary (%d anchors; %d jobs differ from the built-in picker); %d of %d differ from rem.align's final text"
              % (out["check_bad_jobs"], a.jobs, out["anchors"], out["differ_from_builtin"], bad, nrem))
    print(json.dumps(out))
    return 1 if out.get("check_bad_jobs") or out.get("check_bad_rem_jobs") or out.get("digest_bad_jobs") else 0


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
    ap.add_argument("--seqs", type=int, default=2, help="sequences per job")
    ap.add_argument("--multi", choices=("0", "1", "ab"), default=None, help="RV_MANY_MULTI of the many side; ab: off against on, no loop")
    ap.add_argument("--large", choices=("0", "1", "ab"), default=None, help="RV_MANY_LARGE of the many side; ab: off against on, no loop")
    ap.add_argument("--large-multi", choices=("0", "1", "ab"), default=None, help="RV_MANY_LARGE_MULTI of the many side; ab: off against on, no loop")
    ap.add_argument("--large-max", type=int, default=None, help="RV_MANY_LARGE_MAX")
    ap.add_argument("--large-min", type=int, default=None, help="RV_MANY_LARGE_MIN")
    ap.add_argument("--wide", choices=("0", "1", "ab"), default=None, help="RV_MANY_WIDE of the many side; ab: off against on, no loop")
    ap.add_argument("--wide-large-min", type=int, default=None, help="RV_MANY_WIDE_LARGE_MIN")
    ap.add_argument("--sites", action="store_true", help="jobs of --seqs K > 2 sequences: variant sites in subsets of the members, not 1 %% per member")
    ap.add_argument("--no-cut", action="store_true", help="leave lmax as given when jobs of --seqs K sequences pass 2048 ranks")
    ap.add_argument("--picker", action="store_true", help="the reference's default picker: RV_MANY_CHAIN on / off, the built-in picker, rem.align per job; no loop")
    ap.add_argument("--rem-jobs", type=int, default=1000, help="--picker: jobs of the rem.align loop")
    ap.add_argument("--chain-wide", action="store_true", help="--picker for jobs of --seqs K = 17 .. 64 sequences: RV_MANY_CHAIN_WIDE on / off, the built-in picker with RV_MANY_WIDE")
    ap.add_argument("--chain-large", action="store_true", help="--picker for pair jobs above 2048 ranks: RV_MANY_CHAIN_LARGE on / off, the built-in picker with RV_MANY_LARGE")
    ap.add_argument("--chain-large-min", type=int, default=None, help="RV_MANY_CHAIN_LARGE_MIN")
    ap.add_argument("--chain-large-multi", action="store_true", help="--picker for jobs of --seqs K = 3 .. 16 sequences above 2048 ranks: RV_MANY_CHAIN_LARGE_MULTI on / off, the built-in picker with RV_MANY_LARGE_MULTI")
    ap.add_argument("--chain-large-multi-min", type=int, default=None, help="RV_MANY_CHAIN_LARGE_MULTI_MIN")
    ap.add_argument("--chain-wide-large", action="store_true", help="--picker for jobs of --seqs K = 17 .. 64 sequences above 2048 ranks: RV_MANY_CHAIN_WIDE_LARGE on / off, the built-in picker with RV_MANY_WIDE")
    ap.add_argument("--chain-wide-large-min", type=int, default=None, help="RV_MANY_CHAIN_WIDE_LARGE_MIN")
    ap.add_argument("--maxmums", type=int, default=10000, help="--picker: the picker's maxmums (rem.align's default)")
    ap.add_argument("--seedsize", type=int, default=10000, help="--picker: the picker's seedsize (rem.align's default)")
    ap.add_argument("--save-digests", default=None, help="--picker: write a digest per job of the picker side's anchors to this file")
    ap.add_argument("--compare-digests", default=None, help="--picker: count the jobs whose digest differs from this file's")
    ap.add_argument("--mums", action="store_true", help="the match lists (Batch.scan): the shared path, RV_MANY_SCAN_ORDINARY, and the loop through one handle")
    ap.add_argument("--mums-large", action="store_true", help="the match lists of jobs above 2048 ranks: RV_MANY_SCAN_LARGE on, off, and the loop through one handle")
    ap.add_argument("--kchain", action="store_true", help="the collinear chains (Batch.kchain): on the device, RV_MANY_KCHAIN_HOST, and scan + kchain_python per job")
    ap.add_argument("--large-scan", action="store_true", help="--kchain: RV_MANY_SCAN_LARGE on in every leg (jobs above 2048 ranks)")
    ap.add_argument("--python-jobs", type=int, default=None, help="--kchain: kchain_python on the first N jobs only, scaled")
    ap.add_argument("--kchain-big", action="store_true", help="the chaining programme in device memory against RV_MANY_KCHAIN_BIG = 0: abstract lists, 16 lists a call, chain_recurse")
    ap.add_argument("--kb-ks", default="2,3,8", help="--kchain-big: the k of the abstract lists")
    ap.add_argument("--kb-logm", default="8,17", help="--kchain-big: m = 2^lo .. 2^hi")
    ap.add_argument("--kb-host-once", type=float, default=2.0, help="--kchain-big: a host leg expected above this many seconds runs once")
    ap.add_argument("--kb-host-skip", type=float, default=30.0, help="--kchain-big: a host leg expected above this many seconds is left out")
    ap.add_argument("--kb-budget", type=float, default=300.0, help="--kchain-big: seconds after which the sweep over m stops")
    ap.add_argument("--kb-recurse", type=int, default=1000000, help="--kchain-big: bases of the two genomes of the chain_recurse workload (0: none)")
    ap.add_argument("--kb-only", choices=("lists", "many", "recurse"), default=None, help="--kchain-big: one workload")
    ap.add_argument("--sweep", action="store_true", help="--mums-large: then on against off at 1, 2, 4, 8 and 16 jobs a call")
    a = ap.parse_args()
    if a.kchain_big:
        return main_kchain_big(a)
    if a.mums_large:
        a.mums = True
        a.no_cut = True
    if a.kchain and a.large_scan:
        a.no_cut = True
    if a.mums and (a.picker or a.chain_wide or a.chain_large or a.chain_large_multi or a.chain_wide_large or "ab" in (a.multi, a.large, a.large_multi, a.wide)):
        ap.error("--mums is a mode of its own")
    if a.chain_wide_large:
        if not 17 <= a.seqs <= 64:
            ap.error("--chain-wide-large times jobs of 17 .. 64 sequences: --seqs K")
        a.picker = True
        a.no_cut = True
    elif a.chain_wide:
        if not 17 <= a.seqs <= 64:
            ap.error("--chain-wide wants jobs of 17 .. 64 sequences: --seqs K")
        a.picker = True
    elif a.chain_large:
        if a.seqs != 2:
            ap.error("--chain-large times pair jobs")
        a.picker = True
    elif a.chain_large_multi:
        if not 3 <= a.seqs <= 16:
            ap.error("--chain-large-multi times jobs of 3 .. 16 sequences: --seqs K")
        a.picker = True
        a.no_cut = True
    elif a.picker and not 2 <= a.seqs <= 16:
        ap.error("--picker times jobs of 2 .. 16 sequences (17 .. 64: --chain-wide)")
    if [a.multi, a.large, a.large_multi, a.wide].count("ab") > 1:
        ap.error("one switch at a time: --multi ab, --large ab, --large-multi ab or --wide ab")
    if a.wide is not None and not 17 <= a.seqs <= 64:
        ap.error("--wide wants jobs of 17 .. 64 sequences: --seqs K")
    if a.large_multi is not None and a.seqs < 3:
        ap.error("--large-multi wants jobs of three and more sequences: --seqs K")
    jobs = workload(a.jobs, a.lmin, a.lmax, seqs=a.seqs, cut=a.large_multi is None and not a.no_cut, sites=a.sites)
    bases = sum(len(s) for j in jobs for s in j)
    if a.kchain:
        return main_kchain(a, jobs, bases)
    if a.mums_large:
        return main_mums_large(a, jobs, bases)
    if a.mums:
        return main_mums(a, jobs, bases)
    if a.picker:
        return main_picker(a, jobs, bases)
    if a.multi == "ab":
        return main_ab(a, jobs, bases)
    if a.large == "ab":
        return main_ab(a, jobs, bases, "RV_MANY_LARGE")
    if a.large_multi == "ab":
        return main_ab(a, jobs, bases, "RV_MANY_LARGE_MULTI")
    if a.wide == "ab":
        return main_ab(a, jobs, bases, "RV_MANY_WIDE")
    t_loop, t_many, t_many_py = [], [], []
    idx = reveallib.index() if a.only != "many" else None
    batch = None
    if a.only != "loop":
        from reveal_amd import many      # (not needed by --only loop: that side also runs from a checkout without the module)
        batch = many.Batch(False)
        if a.wave_max is not None:
            batch.option("RV_MANY_WAVE_MAX", a.wave_max)
        if a.multi is not None:
            batch.option("RV_MANY_MULTI", int(a.multi))
        if a.large is not None:
            batch.option("RV_MANY_LARGE", int(a.large))
        if a.large_multi == "1":
            batch.option("RV_MANY_LARGE_MULTI", 1)
        elif a.large_multi == "0":
            try:
                batch.option("RV_MANY_LARGE_MULTI", 0)
            except many.error:      # (RV_LIB_DIR: a build from before the switch -- off is all it knows)
                pass
        if a.wide is not None:
            batch.option("RV_MANY_WIDE", int(a.wide))
        more_options(a, batch)
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
    out = dict(jobs=a.jobs, seqs=a.seqs, lmin=a.lmin, lmax=a.lmax, bases=bases, minlength=a.minlength, reps=a.reps, lib_dir=os.environ.get("RV_LIB_DIR", ""))
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
        bad = 0
        for got, (ll, lp, lo) in zip(as_lists(*many_res), loop_res):
            ref = sorted((int(ll[k]), tuple(int(x) for x in lp[lo[k]:lo[k + 1]])) for k in range(len(ll)))
            bad += got != ref
        out["check_bad_jobs"] = bad
        print("check : %d of %d jobs differ between the two sides" % (bad, a.jobs))
    print(json.dumps(out))
    return 1 if out.get("check_bad_jobs") else 0


if __name__ == "__main__":
    sys.exit(main())
