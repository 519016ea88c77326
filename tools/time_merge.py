#!/usr/bin/env python3
"""merge_consecutive on the device against the host leg it replaces, and what keeping the block list in columns is worth: the chains the glocal filter
leaves of two synthetic genomes (tools/time_glocal.py's lists: synth.genomes, 1 % variants; the SNP class, and the indel class with a fifth of the
variants indels; the query in contigs of which every third is reverse-complemented), with the command line's weights.

    python tools/time_merge.py [--sizes 5000000,250000000] [--classes indel,snp] [--nocluster-sizes 5000000] [--contigs 8] [--reps 5] [--sweep]
                               [--pipeline 5000000] [--optimise 2000] [--out FILE]

Legs, A and B alternately on one handle, `reps` times each after a warm-up of both:
  A   the kernels (RV_MERGE_HOST_BELOW = 0)
  B   RV_MERGE_HOST = 1: the rule in host C++ inside the same call
The times are those of transform.merge_arrays(cols, sel = the filter's chain) on the columns in front of the filter: what transform.synteny_layout calls.
Prints medians, spreads (max - min), the gate -- A's median below B's by more than the sum of the two spreads -- and the call's own info.  A and B must
give the same rows.  --sweep: the first list's chain cut to its first k entries, on columns of those k rows with sel = 0 .. k - 1, k = 2^6 .. 2^19,
five runs a leg: the smallest k from which the gate holds at every longer k is what RV_MERGE_HOST_BELOW should be.  --pipeline L: synteny_layout
against synteny_chain + chain_tail on tuples, 2 x L bases.  --optimise N: rv_optimise_host against optimise_python on a fragmented list of N blocks
(host only).  Exit status 1 when the legs differ (a missed gate is a finding, not a failure)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reveal_amd import transform      # noqa: E402

W = transform.TRANSFORM_DEFAULTS
RC = bytes.maketrans(b"ACGT", b"TGCA")
COLS = [k for k, _ in transform._COLS]


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def legs(idx, cols, sel, reps):
    t, last = {"A": [], "B": []}, {}
    for rep in range(reps + 1):      # (the first round of both is the warm-up: allocations)
        for name in ("A", "B"):
            idx.set_option("RV_MERGE_HOST", 1 if name == "B" else 0)
            dt, r = timed(lambda: transform.merge_arrays(cols, sel, index=idx))
            if rep:
                t[name].append(dt)
            last[name] = r
    idx.set_option("RV_MERGE_HOST", 0)
    same = all(np.array_equal(last["A"][0][k], last["B"][0][k]) for k in COLS)
    med = {k: statistics.median(v) for k, v in t.items()}
    spr = {k: max(v) - min(v) for k, v in t.items()}
    return t, med, spr, bool(med["A"] < med["B"] - (spr["A"] + spr["B"])), bool(same), last["A"][1], last["B"][1]


def contigs_of(qry, contigs):
    step = len(qry) // contigs + 1
    return [qry[k * step:(k + 1) * step].translate(RC)[::-1] if k % 3 == 2 else qry[k * step:(k + 1) * step] for k in range(contigs)]


def fragmented(n, seed=11):
    """a chain as a fragmented draft leaves it: runs of one to three blocks, every run on a contig and in an orientation of its own"""
    rng, out, k = random.Random(seed), [], 0
    while k < n:
        L = min(rng.randint(1, 3), n - k)
        o, ctg = rng.randrange(2), 1 + rng.randrange(3)
        for j in range(L):
            a = 1000 + 100 * (k + j)
            b = 1000000 + 100 * (k + j) if o == 0 else 1000000 + 100 * (k + L - 1 - j)
            out.append((a, a + rng.randint(10, 90), b, b + rng.randint(10, 90), o, rng.randint(1, 500), 0, ctg))
        k += L
    ranges = [(0, 999999), (1000000, 1999999), (2000000, 2999999), (3000000, 3999999)]
    return out, ranges, 999999, 3000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000000,250000000")
    ap.add_argument("--classes", default="indel,snp")
    ap.add_argument("--nocluster-sizes", default="5000000", help="sizes at which the list of one block per MUM is timed too")
    ap.add_argument("--contigs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--pipeline", default="")
    ap.add_argument("--optimise", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines, results, ok = [], [], True

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if a.optimise:
        blocks, ranges, rl, ql = fragmented(a.optimise)
        kw = {k: W[k] for k in transform._W}
        tn, native = timed(lambda: transform.optimise_native(blocks, rl, ql, ranges, **kw))
        tp, python = timed(lambda: transform.optimise_python(blocks, rl, ql, ranges, **kw))
        ok = ok and native == python
        say("one sweep of optimise on %d blocks (%d kept): rv_optimise_host %.4f s, optimise_python %.2f s, ratio %.0f; same result: %s"
            % (len(blocks), len(native[0]), tn, tp, tp / tn, native == python))
    sizes = [int(x) for x in a.sizes.split(",") if x]
    if sizes or a.pipeline:
        from reveal_amd import reveallib, synth
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from time_glocal import block_columns
    first = None
    if sizes:
        idx = reveallib.index()
        say("weights %s; RV_MERGE_HOST_BELOW as shipped %d" % (W, idx.get_option("RV_MERGE_HOST_BELOW")))
        idx.set_option("RV_MERGE_HOST_BELOW", 0)
        nocl = [int(x) for x in a.nocluster_sizes.split(",") if x]
        for L in sizes:
            for cls in a.classes.split(","):
                for cluster in [True] + ([False] if L in nocl and cls == "indel" else []):
                    dt, (cols, ranges, rlength, mums) = timed(lambda: block_columns(L, 0.2 if cls == "indel" else 0.0, a.contigs, cluster))
                    df, (sel, ginfo) = timed(lambda: transform.glocal_arrays(cols, rlength, ranges, (0, 1), True, index=idx, **W))
                    say("2 x %d %s%s, query in %d contigs: %d blocks (made in %.1f s) -> the filter (%s, %.3f s) leaves %d" % (
                        L, cls, "" if cluster else " nocluster", a.contigs, len(cols["s1"]), dt, ginfo["route"], df, len(sel)))
                    if first is None or len(sel) > len(first[1]):
                        first = (cols, sel)
                    t, med, spr, gate, same, info, binfo = legs(idx, cols, sel, a.reps)
                    ok = ok and same
                    for k in ("A", "B"):
                        say("    %s  runs %s s; median %.5f s, spread %.5f s" % (k, " ".join("%.5f" % x for x in t[k]), med[k], spr[k]))
                    say("    gate (A < B - both spreads): %s; ratio B / A %.2f; same rows: %s" % ("met" if gate else "MISSED", med["B"] / med["A"], same))
                    say("    A: %d rows in, %d out; key bits %s, %d launches of its own, %.3f ms between the events; %d bytes up, %d bytes down" % (
                        info["rows_in"], info["rows_out"], info["key_bits"], info["launches"], info["kernel_ms"], info["bytes_up"], info["bytes_down"]))
                    results.append(dict(L=L, cls=cls, cluster=cluster, blocks=len(cols["s1"]), chain=len(sel), A_s=t["A"], B_s=t["B"], A_median_s=med["A"], B_median_s=med["B"],
                                        A_spread_s=spr["A"], B_spread_s=spr["B"], gate=gate, same=same, info=info))
        if a.sweep and first is not None:
            cols, sel = first
            say("sweep: the first k entries of the longest chain as a list of their own (columns of k rows, sel = 0 .. k - 1), %d runs a leg after a warm-up" % a.reps)
            holds = []
            for e in range(6, 20):
                k = 1 << e
                if k > len(sel):
                    break
                sub = {c: np.ascontiguousarray(np.asarray(cols[c])[sel[:k]]) for c in COLS}
                t, med, spr, gate, same, info, binfo = legs(idx, sub, np.arange(k, dtype=np.int32), a.reps)
                ok = ok and same
                holds.append((k, gate))
                say("  k = %6d: A %.6f s (spread %.6f), B %.6f s (spread %.6f), B / A %.2f, gate %s; %d rows out, %.3f ms between the events; same rows: %s" % (
                    k, med["A"], spr["A"], med["B"], spr["B"], med["B"] / med["A"], "met" if gate else "MISSED", info["rows_out"], info["kernel_ms"], same))
            from_k = None
            for k, gate in reversed(holds):
                if not gate:
                    break
                from_k = k
            say("the gate holds from k = %s on" % (from_k if from_k is not None else "nowhere"))
    for L in [int(x) for x in a.pipeline.split(",") if x]:
        ref, qry = synth.genomes(L, 2, indelfrac=0.2)
        ctgs = contigs_of(qry, a.contigs)
        t = {"columns": [], "tuples": []}
        try:
            transform.synteny_layout([ref], ctgs)
        except transform.error as e:      # (the reference raises on such a chain too: nothing to time behind the merge)
            say("pipeline, 2 x %d indel: the tail raises on this chain (%s)" % (L, e))
            continue
        for rep in range(4):
            dc, lay = timed(lambda: transform.synteny_layout([ref], ctgs))
            dt1, chain = timed(lambda: transform.synteny_chain([ref], ctgs))
            dt2, tail = timed(lambda: transform.chain_tail(chain["chain"], chain["rlength"], chain["qlength"], chain["ctg2range"]))
            same = all(lay[k] == tail[k] for k in ("blocks", "weight", "cost", "edgecosts", "extended"))
            ok = ok and same
            if rep:
                t["columns"].append(dc)
                t["tuples"].append(dt1 + dt2)
        say("pipeline, 2 x %d indel: %d blocks -> chain of %d -> %d merged -> %d in the layout; synteny_layout (columns, merge route %s) median %.3f s (runs %s); "
            "synteny_chain + chain_tail (tuples) median %.3f s (runs %s; the tail alone %.4f s); same result: %s" % (
                L, len(chain["blocks"]), len(chain["chain"]), lay["info"]["merge"]["rows_out"], len(lay["blocks"]), lay["info"]["merge"]["route"],
                statistics.median(t["columns"]), " ".join("%.3f" % x for x in t["columns"]), statistics.median(t["tuples"]), " ".join("%.3f" % x for x in t["tuples"]), dt2, same))
    say(json.dumps(dict(results=results, ok=bool(ok))))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
