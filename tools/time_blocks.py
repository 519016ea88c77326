#!/usr/bin/env python3
"""getblocks against the routes it replaces, on the GPU: the call AFTER construct on two synthetic genomes (synth.genomes, 1 % variants; the SNP
class, and the indel class with a fifth of the variants indels), under construct(rc=0) and construct(rc=1).

    python tools/time_blocks.py [--sizes 5000000,250000000] [--reps 5] [--no-python] [--out FILE]

Legs, A, B and S alternately on one handle, `reps` times each after a warm-up of all:
  A   index.getblocks_arrays with RV_BLOCKS_HOST_BELOW = 0: the MUMs stay in device memory whatever their number, the blocks come back
  B   the same call with RV_BLOCKS_HOST = 1: every MUM crosses as for getmums, then the rule in host C++ -- the strict baseline
  S   the same call as shipped: below RV_BLOCKS_HOST_BELOW records the host rule (the records arrive with the header's copy), the kernels otherwise
  C   index.getmums + transform.blocks_python, ONE run: what a caller does without getblocks
Prints medians, spreads (max - min), the bytes each leg copies back (from the counts: the scan's header and records of 16 B -- 24 B in the 64-bit
library --, or the header, 16 B of counts and 48 B a kept block) and the gate: A's median below B's by more than the sum of the two spreads.  A and B
must give the same arrays.  Exit status 1 when a gate is missed."""
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
ARGS = (20, True, 30, 50)      # `reveal transform`'s defaults


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000000,250000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-python", action="store_true", help="leave leg C out")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines, results, ok = [], [], True

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for L in [int(x) for x in a.sizes.split(",")]:
        for cls, indelfrac in (("snp", 0.0), ("indel", 0.2)):
            seqs = synth.genomes(L, 2, indelfrac=indelfrac)
            idx = reveallib.index()
            shipped = idx.get_option("RV_BLOCKS_HOST_BELOW")
            ranges = []
            for k, s in enumerate(seqs):
                idx.addsample("g%d" % k)
                ranges.append(idx.addsequence(s))
            del seqs
            for rc in (0, 1):
                idx.construct(rc=rc)
                legs = {"A": (0, 0), "B": (1, 0), "S": (0, shipped)}
                t = {"A": [], "B": [], "S": []}
                last = {}
                for rep in range(a.reps + 1):      # (the first round of all is the warm-up: allocations, the capacity retry)
                    for name, (sw, below) in legs.items():
                        idx.set_option("RV_BLOCKS_HOST", sw)
                        idx.set_option("RV_BLOCKS_HOST_BELOW", below)
                        dt, r = timed(lambda: idx.getblocks_arrays(*ARGS))
                        if rep:
                            t[name].append(dt)
                        last[name] = r
                idx.set_option("RV_BLOCKS_HOST", 0)
                idx.set_option("RV_BLOCKS_HOST_BELOW", shipped)
                same = all(np.array_equal(last["A"][k], last["S"][k]) for k in KEYS) and last["A"]["info"] == last["B"]["info"] and all(np.array_equal(last["A"][k], last["B"][k]) for k in KEYS)
                info = last["A"]["info"]
                nb = len(last["A"]["s1"])
                med = {k: statistics.median(v) for k, v in t.items()}
                spr = {k: max(v) - min(v) for k, v in t.items()}
                gate = med["A"] < med["B"] - (spr["A"] + spr["B"])
                ok = ok and gate and same
                rec = dict(L=L, cls=cls, rc=rc, mums=info["mums"], clusters=info["clusters"], blocks=nb, A_s=t["A"], B_s=t["B"], A_median_s=med["A"], B_median_s=med["B"],
                           A_spread_s=spr["A"], B_spread_s=spr["B"], gate=bool(gate), same=bool(same),
                           A_bytes_back=16 + 16 + 48 * nb, B_bytes_back=16 * (info["mums"] + 1))
                say("2 x %d %s rc=%d: %d MUMs -> %d clusters -> %d blocks" % (L, cls, rc, info["mums"], info["clusters"], nb))
                host_rule = info["mums"] < shipped
                rec.update(S_s=t["S"], S_median_s=med["S"], S_spread_s=spr["S"], S_host_rule=bool(host_rule), S_bytes_back=16 * (min(info["mums"], shipped) + 1) + (0 if host_rule else 16 + 48 * nb))
                for k in ("A", "B", "S"):
                    say("  %s  runs %s s; median %.5f s, spread %.5f s; %d bytes copied back%s" % (k, " ".join("%.5f" % x for x in t[k]), med[k], spr[k], rec[k + "_bytes_back"],
                                                                                               " (threshold %d: %s)" % (shipped, "host rule" if host_rule else "kernels") if k == "S" else ""))
                say("  gate (A < B - both spreads): %s; ratio B / A %.2f; same arrays: %s" % ("met" if gate else "MISSED", med["B"] / med["A"], same))
                if not a.no_python:
                    dt, blocks = timed(lambda: transform.blocks_python(idx.getmums(ARGS[0]), ranges, ARGS[1], ARGS[2], ARGS[3], rcmums=bool(rc)))
                    cols = [last["A"][k].tolist() for k in KEYS]
                    same_c = blocks == [(s1, e1, s2, e2, rc, sc, rf, cg) for s1, e1, s2, e2, sc, rf, cg in zip(*cols)]
                    ok = ok and same_c
                    rec.update(C_s=dt, C_same=bool(same_c))
                    say("  C  one run %.3f s (getmums + blocks_python); same list: %s" % (dt, same_c))
                results.append(rec)
            del idx
    say(json.dumps(dict(results=results, ok=bool(ok))))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
