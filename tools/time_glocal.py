#!/usr/bin/env python3
"""The glocal chain against the host leg it replaces, on the GPU: the block lists of two synthetic genomes (synth.genomes, 1 % variants; the SNP class,
and the indel class with a fifth of the variants indels), the query cut into contigs of which every third is reverse-complemented, forward and
reverse-complement blocks joined as transform.synteny_blocks joins them -- with the command line's weights.

    python tools/time_glocal.py [--sizes 5000000,250000000] [--classes snp,indel] [--nocluster] [--contigs 8] [--reps 5] [--python-below 20000]
                                [--sweep] [--out FILE]

Legs, A and B alternately on one handle, `reps` times each after a warm-up of both, for ONE PASS on the reference axis and for THE FILTER (both loops):
  A   the kernels (RV_GLOCAL_HOST_BELOW = 0)
  B   RV_GLOCAL_HOST = 1: the rule in host C++ inside the same call
  P   transform.glocalchain_python, one pass, ONE run, on lists below --python-below blocks: for scale
The times are those of transform.glocal_arrays on columns (no Python list is built).  Prints medians, spreads (max - min), the gate -- A's median below
B's by more than the sum of the two spreads --, and from the call's own info: passes per axis, tiles, edges, the recurrence kernel's time per entry
(events round its launches) and the bytes copied.  A and B must give the same chain.  --sweep: the filter on prefixes of the first list in sorted
order, lengths 2^8 .. 2^17, three runs a leg: where A starts to win.  Exit status 1 when chains differ (a missed gate is a finding, not a failure)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reveal_amd import reveallib, synth, transform      # noqa: E402

KEYS = ("s1", "e1", "s2", "e2", "score", "refid", "ctgid")
W = transform.TRANSFORM_DEFAULTS
RC = bytes.maketrans(b"ACGT", b"TGCA")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def block_columns(L, indelfrac, contigs, cluster):
    """-> (columns, ctg2range, rlength, (forward, reverse-complement) MUMs)"""
    ref, qry = synth.genomes(L, 2, indelfrac=indelfrac)
    idx = reveallib.index()
    idx.set_option("RV_BLOCKS_HOST_BELOW", 0)
    ranges = []
    idx.addsample("reference")
    ranges.append(idx.addsequence(ref))
    idx.addsample("contigs")
    step = len(qry) // contigs + 1
    for k in range(contigs):
        c = qry[k * step:(k + 1) * step]
        ranges.append(idx.addsequence(c.translate(RC)[::-1] if k % 3 == 2 else c))
    del ref, qry
    parts, mums = [], []
    for rc in (0, 1):
        idx.construct(rc=rc)
        r = idx.getblocks_arrays(20, cluster, 30, 50)
        r["o"] = np.full(len(r["s1"]), rc, dtype=np.int32)
        parts.append(r)
        mums.append(r["info"]["mums"])
    cols = {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in KEYS + ("o",)}
    return cols, ranges, idx.nsep[0], tuple(mums)


def legs(idx, cols, ranges, rlength, reps, fixed, say, what):
    t, last = {"A": [], "B": []}, {}
    for rep in range(reps + 1):      # (the first round of both is the warm-up: allocations)
        for name in ("A", "B"):
            idx.set_option("RV_GLOCAL_HOST", 1 if name == "B" else 0)
            dt, r = timed(lambda: transform.glocal_arrays(cols, rlength, ranges, (0, 1) if fixed else (0,), fixed, index=idx, **W))
            if rep:
                t[name].append(dt)
            last[name] = r
    idx.set_option("RV_GLOCAL_HOST", 0)
    same = np.array_equal(last["A"][0], last["B"][0]) and last["A"][1]["after"] == last["B"][1]["after"]
    med = {k: statistics.median(v) for k, v in t.items()}
    spr = {k: max(v) - min(v) for k, v in t.items()}
    gate = med["A"] < med["B"] - (spr["A"] + spr["B"])
    info = last["A"][1]
    say("  %s: %d blocks -> %d; passes %s, left after each %s" % (what, len(cols["s1"]), len(last["A"][0]), info["passes"], info["after"]))
    for k in ("A", "B"):
        say("    %s  runs %s s; median %.4f s, spread %.4f s" % (k, " ".join("%.4f" % x for x in t[k]), med[k], spr[k]))
    say("    gate (A < B - both spreads): %s; ratio B / A %.2f; same chain: %s" % ("met" if gate else "MISSED", med["B"] / med["A"], same))
    per = info["chain_ms"] * 1e6 / info["chain_blocks"] if info["chain_blocks"] else float("nan")
    say("    A: %d tiles (most in a pass %d), %d edges, sort keys %d; recurrence kernel %.2f ms over %d entries = %.1f ns an entry, %.1f an edge; %d bytes up, %d bytes down"
        % (info["tiles"], info["tiles_max"], info["edges"], info["sort_keys"], info["chain_ms"], info["chain_blocks"], per,
           info["chain_ms"] * 1e6 / max(info["edges"], 1), info["bytes_up"], info["bytes_down"]))
    return dict(what=what, blocks=len(cols["s1"]), left=len(last["A"][0]), A_s=t["A"], B_s=t["B"], A_median_s=med["A"], B_median_s=med["B"], A_spread_s=spr["A"],
                B_spread_s=spr["B"], gate=bool(gate), same=bool(same), info=info), bool(same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000000,250000000")
    ap.add_argument("--classes", default="snp,indel")
    ap.add_argument("--nocluster", action="store_true", help="one block per MUM (reveal transform --nocluster)")
    ap.add_argument("--contigs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--python-below", type=int, default=20000)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines, results, ok = [], [], True

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    idx = reveallib.index()
    say("weights %s; RV_GLOCAL_HOST_BELOW as shipped %d, RV_GLOCAL_EDGE_BUDGET %d" % (W, idx.get_option("RV_GLOCAL_HOST_BELOW"), idx.get_option("RV_GLOCAL_EDGE_BUDGET")))
    idx.set_option("RV_GLOCAL_HOST_BELOW", 0)
    first = None
    for L in [int(x) for x in a.sizes.split(",")]:
        for cls in a.classes.split(","):
            dt, (cols, ranges, rlength, mums) = timed(lambda: block_columns(L, 0.2 if cls == "indel" else 0.0, a.contigs, not a.nocluster))
            n = len(cols["s1"])
            say("2 x %d %s%s, query in %d contigs: %s MUMs -> %d blocks (%d with o = 1; made in %.1f s)" % (L, cls, " nocluster" if a.nocluster else "", a.contigs, mums, n,
                                                                                                      int(cols["o"].sum()), dt))
            if first is None:
                first = (cols, ranges, rlength)
            for fixed in (False, True):
                rec, same = legs(idx, cols, ranges, rlength, a.reps, fixed, say, "the filter" if fixed else "one pass, axis 0")
                rec.update(L=L, cls=cls, cluster=not a.nocluster)
                results.append(rec)
                ok = ok and same
                flush()
            if n < a.python_below:
                blocks = list(zip(*[cols[k].tolist() for k in ("s1", "e1", "s2", "e2", "o", "score", "refid", "ctgid")]))
                dt, chain = timed(lambda: transform.glocalchain_python(blocks, rlength, 0, ranges, axis=0, **W))
                one = transform.glocal_arrays(cols, rlength, ranges, (0,), False, index=idx, **W)[0]
                same = [blocks[i] for i in one.tolist()] == chain
                ok = ok and same
                say("  P  one pass, axis 0, one run %.2f s (glocalchain_python, %.0f blocks a second); same chain: %s" % (dt, n / dt, same))
                flush()
    if a.sweep and first is not None:
        cols, ranges, rlength = first
        order = np.argsort(cols["s1"], kind="stable")
        say("sweep: the filter on the first k blocks of the first list in reference order, three runs a leg after a warm-up, medians")
        for e in range(8, 18):
            k = 1 << e
            if k > len(order):
                break
            sub = {c: np.ascontiguousarray(v[order[:k]]) for c, v in cols.items()}
            t = {"A": [], "B": []}
            for rep in range(4):
                for name in ("A", "B"):
                    idx.set_option("RV_GLOCAL_HOST", 1 if name == "B" else 0)
                    dt, r = timed(lambda: transform.glocal_arrays(sub, rlength, ranges, (0, 1), True, index=idx, **W))
                    if rep:
                        t[name].append(dt)
            idx.set_option("RV_GLOCAL_HOST", 0)
            say("  k = %6d: A %.5f s, B %.5f s, B / A %.2f; passes %s" % (k, statistics.median(t["A"]), statistics.median(t["B"]), statistics.median(t["B"]) / statistics.median(t["A"]),
                                                                        r[1]["passes"]))
            flush()
    say(json.dumps(dict(results=results, ok=bool(ok))))
    flush()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
