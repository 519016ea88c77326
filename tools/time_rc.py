#!/usr/bin/env python3
"""construct(rc=1) with the reverse complement made in device memory against the host loop plus second upload, on one GPU, 32-bit library.

    python tools/time_rc.py [--parts ab,kernel,sweep,e2e] [--sizes 250000000,5000000,300] [--reps 5] [--out FILE]

  ab      two handles on the same two synthetic genomes (synth.genomes, 1 % variants), construct(rc=0) done on both: A = construct(rc=1) on the
          device leg (RV_RC_HOST_BELOW = 0), B = the same call with RV_RC_HOST = 1; alternately, `reps` times each after one warm-up round.  Every
          call flips the text, the same work each time.  Gate: A's median below B's by more than the sum of the two spreads (max - min).
  kernel  k_text_revcomp alone on the range of 2 x the first size, and a device-to-device copy of as many bytes, between HIP events in one run
          (rv_test_revcomp_time): medians and their ratio, no gate.
  sweep   `ab` over range lengths of 100 x 4^k bytes up to 26 MB, and 64 MiB, behind a reference of 100 bases: where, if anywhere, B wins.
  e2e     transform.synteny_blocks on 2 x the first size, sequences in, blocks out, `reps` times after a warm-up (run it from a checkout of the
          parent commit as well, in turn).
Exit status 1 when an `ab` gate is missed."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reveal_amd import _lib, reveallib, synth, transform      # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def handle(seqs, host):
    idx = reveallib.index()
    for k, s in enumerate(seqs):
        idx.addsample("g%d" % k)
        idx.addsequence(s)
    idx.set_option("RV_RC_HOST", 1 if host else 0)
    idx.set_option("RV_RC_HOST_BELOW", 0)
    idx.construct(rc=0)
    return idx


def ab(seqs, reps):
    """-> dict of the two legs' times, medians, spreads and the gate"""
    legs = {"A": handle(seqs, False), "B": handle(seqs, True)}
    t = {"A": [], "B": []}
    for rep in range(reps + 1):      # (the first round is the warm-up)
        for name, idx in legs.items():
            dt = timed(lambda: idx.construct(rc=1))
            if rep:
                t[name].append(dt)
    info = {k: idx.text_info() for k, idx in legs.items()}
    same = np.array_equal(legs["A"].array("SA"), legs["B"].array("SA")) and np.array_equal(legs["A"].array("T"), legs["B"].array("T"))
    med = {k: statistics.median(v) for k, v in t.items()}
    spr = {k: max(v) - min(v) for k, v in t.items()}
    return dict(A_s=t["A"], B_s=t["B"], A_median_s=med["A"], B_median_s=med["B"], A_spread_s=spr["A"], B_spread_s=spr["B"],
                gate=bool(med["A"] < med["B"] - (spr["A"] + spr["B"])), same=bool(same), A_uploads=info["A"]["uploads"], B_uploads=info["B"]["uploads"],
                A_rc_device=info["A"]["rc_device"], B_rc_device=info["B"]["rc_device"])


def show(say, r):
    for k in ("A", "B"):
        say("  %s  runs %s ms; median %.3f ms, spread %.3f ms; %d uploads, rc_device %d" % (k, " ".join("%.3f" % (1e3 * x) for x in r[k + "_s"]), 1e3 * r[k + "_median_s"],
                                                                                         1e3 * r[k + "_spread_s"], r[k + "_uploads"], r[k + "_rc_device"]))
    say("  gate (A < B - both spreads): %s; ratio B / A %.2f; same SA and T: %s" % ("met" if r["gate"] else "MISSED", r["B_median_s"] / r["A_median_s"], r["same"]))
    # the text alternates between two states (contigs reversed, contigs forward) whose index costs differently to build: the same figures per state, no gate
    for name, sl in (("odd repetitions", slice(0, None, 2)), ("even repetitions", slice(1, None, 2))):
        x, y = r["A_s"][sl], r["B_s"][sl]
        if x and y:
            say("  %s: A %.3f .. %.3f ms, B %.3f .. %.3f ms" % (name, 1e3 * min(x), 1e3 * max(x), 1e3 * min(y), 1e3 * max(y)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab,kernel,sweep")
    ap.add_argument("--sizes", default="250000000,5000000,300")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    parts = a.parts.split(",")
    sizes = [int(x) for x in a.sizes.split(",")]
    lines, results, ok = [], {}, True

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if "ab" in parts:
        results["ab"] = []
        for L in sizes:
            seqs = synth.genomes(L, 2)
            r = ab(seqs, a.reps)
            del seqs
            r["L"] = L
            say("construct(rc=1), 2 x %d, range of %d bytes" % (L, L + 2))
            show(say, r)
            ok = ok and r["gate"] and r["same"]
            results["ab"].append(r)
    if "kernel" in parts:
        L = sizes[0]
        n = a.reps
        km, cm = (ctypes.c_double * n)(), (ctypes.c_double * n)()
        lib = _lib.get(False)
        if lib.dll.rv_test_revcomp_time(L, L + 2, n, km, cm) != 0:
            raise RuntimeError(lib.err())
        km, cm = list(km), list(cm)
        r = dict(len=L + 2, lo=L, kernel_ms=km, copy_ms=cm, kernel_median_ms=statistics.median(km), copy_median_ms=statistics.median(cm))
        r["ratio"] = r["kernel_median_ms"] / r["copy_median_ms"]
        r["kernel_tb_s"] = 2 * (L + 2) / (r["kernel_median_ms"] * 1e9)
        r["copy_tb_s"] = 2 * (L + 2) / (r["copy_median_ms"] * 1e9)
        say("k_text_revcomp on %d bytes at text position %d against a device-to-device copy of as many (HIP events)" % (L + 2, L))
        say("  kernel  runs %s ms; median %.4f ms = %.2f TB/s read + written" % (" ".join("%.4f" % x for x in km), r["kernel_median_ms"], r["kernel_tb_s"]))
        say("  copy    runs %s ms; median %.4f ms = %.2f TB/s read + written" % (" ".join("%.4f" % x for x in cm), r["copy_median_ms"], r["copy_tb_s"]))
        say("  kernel / copy %.2f" % r["ratio"])
        results["kernel"] = r
    if "sweep" in parts:
        results["sweep"] = []
        rng = np.random.default_rng(5)
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        lengths = [100 * 4 ** k for k in range(10)] + [64 << 20]
        say("sweep: range length, A median / spread ms, B median / spread ms, B / A")
        for length in lengths:
            ref = acgt[rng.integers(0, 4, 100)].tobytes()
            ctg = acgt[rng.integers(0, 4, length - 2)].tobytes()
            r = ab([ref, ctg], a.reps)
            r["len"] = length
            say("  %9d  A %9.3f / %7.3f  B %9.3f / %7.3f  B / A %.2f%s" % (length, 1e3 * r["A_median_s"], 1e3 * r["A_spread_s"], 1e3 * r["B_median_s"], 1e3 * r["B_spread_s"],
                                                                         r["B_median_s"] / r["A_median_s"], "" if r["same"] else "  DIFFERENT RESULTS"))
            ok = ok and r["same"]
            results["sweep"].append(r)
        losing = [r["len"] for r in results["sweep"] if r["B_median_s"] < r["A_median_s"]]
        say("  lengths at which B's median is below A's: %s" % (losing or "none"))
    if "e2e" in parts:
        L = sizes[0]
        seqs = synth.genomes(L, 2)
        t, text = [], None
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            r = transform.synteny_blocks([seqs[0]], [seqs[1]])
            dt = time.perf_counter() - t0
            text = r.get("text")
            nblocks = len(r["blocks"])
            del r
            if rep:
                t.append(dt)
        say("transform.synteny_blocks, 2 x %d, sequences in, blocks out: runs %s s; median %.3f s, spread %.3f s; %d blocks; text %s" % (
            L, " ".join("%.3f" % x for x in t), statistics.median(t), max(t) - min(t), nblocks, text))
        results["e2e"] = dict(L=L, runs_s=t, median_s=statistics.median(t), spread_s=max(t) - min(t), blocks=nblocks, text=text)
    say(json.dumps(dict(results=results, ok=bool(ok))))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
