#!/usr/bin/env python3
"""Writes tests/golden/many_chain.json: what `reveal refine --method reveal_rem` computes for the jobs of tests/many_chain_cases.py -- `rem.align` with
the reference's default picker (schemes.graphmumpicker) per job, on the REFERENCE's own index module (oracle/_ref/reveallib.so: `make -C oracle &&
make -C oracle refmod`), under every parameter set of the cases module.  Per job and set: the sorted anchors (l, pos_a, pos_b) in the coordinates of the
job's text `a$b$`, and the SHA-256 of the final text.  The sequences are not stored: the cases module regenerates them.  CPU only (the host library is
needed for rv_chain, which schemes.chain calls).

It refuses to write a fixture that tests nothing: under the default set at least half of the `rearranged` jobs must have other anchors than the built-in
picker gives (many_cases.oracle_job), and every other set must change at least 10 of them against the default set."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    import many_cases as mc
    import many_chain_cases as cc
    import pin_oracle
    refmod = pin_oracle.load_refmod(False)
    if refmod is None:
        sys.exit("oracle/_ref/reveallib.so is not built: make -C oracle && make -C oracle refmod")
    jobs = cc.jobs()
    results = {}
    for name, kw in cc.SETS:
        out = []
        for cls, (a, b) in jobs:
            an, T = cc.rem_align_job([a, b], indexmod=refmod, **kw)
            out.append(dict(anchors=[[l, p[0], p[1]] for l, p in an], sha=cc.sha(T)))
        results[name] = out
        print("%-9s %6d anchors" % (name, sum(len(r["anchors"]) for r in out)), file=sys.stderr)
    rea = [j for j, (cls, _) in enumerate(jobs) if cls == "rearranged"]
    builtin = 0
    for j in rea:
        a, b = jobs[j][1]
        want, _ = mc.oracle_job([a.upper().encode(), b.upper().encode()], minl=20)
        builtin += [(l, p) for l, p in want] != [(r[0], (r[1], r[2])) for r in results["default"][j]["anchors"]]
    print("rearranged jobs whose anchors differ from the built-in picker's: %d of %d" % (builtin, len(rea)), file=sys.stderr)
    assert 2 * builtin >= len(rea), "the default picker agrees with the built-in one on most rearranged jobs: the fixture would test nothing"
    for name, _ in cc.SETS[1:]:
        changed = sum(results[name][j]["anchors"] != results["default"][j]["anchors"] for j in rea)
        print("  %-9s changes %d of them against the default set" % (name, changed), file=sys.stderr)
        assert changed >= 10, "set %s changes only %d rearranged jobs" % (name, changed)
    doc = dict(sets=[n for n, _ in cc.SETS], jobs=len(jobs), results=results)
    with open(cc.GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (cc.GOLDEN, os.path.getsize(cc.GOLDEN)), file=sys.stderr)


if __name__ == "__main__":
    main()
