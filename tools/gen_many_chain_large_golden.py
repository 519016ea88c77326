#!/usr/bin/env python3
"""Writes tests/golden/many_chain_large.json: what `reveal refine --method reveal_rem` computes for the jobs of tests/many_chain_large_cases.py -- `rem.align`
with the reference's default picker (schemes.graphmumpicker) per job, on the REFERENCE's own index module (oracle/_ref/reveallib.so: `make -C oracle &&
make -C oracle refmod`), under every parameter set of the cases module, exactly as tools/gen_many_chain_golden.py does for the small pair jobs.  Per job and
set: the sorted anchors (l, pos_a, pos_b) in the coordinates of the job's text `a$b$` and the SHA-256 of the final text; a result an earlier set already has
is kept once ("same").  Also: the first pick of every job under `default` and the number of
matches at every job's root (the CPU oracle's scan), which conditions (c) and (d) below read.  The sequences are not stored.  CPU only.

It refuses to write a fixture that tests nothing:
  (a) under `default` at least half of the `rearranged-large` jobs have other anchors than the built-in picker's (many_cases.oracle_job);
  (b) every other set changes at least 5 of them against `default`;
  (c) by the oracle's match list alone, at least 5 jobs hold more than 64 candidates at the root and at least one more than 256;
  (d) at least 10 jobs have a child of more than 2048 ranks below the root, so the chain pick of the level pipeline also runs below the root.
The file stays below 300 KB."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def conditions(cl, jobs, default, others, roots, candidates, big_candidates, builtin_of):
    """the four conditions on a fixture: default = [sorted anchors] per job, others = {set: [digest per job]} -> list of failures"""
    bad = []
    rea = [j for j, (cls, _) in enumerate(jobs) if cls == "rearranged-large"]
    differ = sum(builtin_of(j) != default[j] for j in rea)
    if 2 * differ < len(rea):
        bad.append("(a) the default picker agrees with the built-in one on %d of %d rearranged-large jobs" % (len(rea) - differ, len(rea)))
    dd = [cl.digest(a) for a in default]
    for name, dig in others.items():
        changed = sum(dig[j] != dd[j] for j in rea)
        if changed < 5:
            bad.append("(b) set %s changes only %d rearranged-large jobs" % (name, changed))
    allc = list(candidates) + [big_candidates]
    if sum(c > 64 for c in allc) < 5 or sum(c > 256 for c in allc) < 1:
        bad.append("(c) %d jobs above 64 candidates at the root, %d above 256" % (sum(c > 64 for c in allc), sum(c > 256 for c in allc)))
    deep = sum(r is not None and max(cl.children_ranks(jobs[j][1], r)) > 2048 for j, r in enumerate(roots))
    if deep < 10:
        bad.append("(d) only %d jobs with a child of more than 2048 ranks" % deep)
    return bad


def main():
    import many_cases as mc
    import many_chain_large_cases as cl
    import pin_oracle
    refmod = pin_oracle.load_refmod(False)
    if refmod is None:
        sys.exit("oracle/_ref/reveallib.so is not built: make -C oracle && make -C oracle refmod")
    jobs = cl.jobs()
    full, roots = {}, []
    for name, kw in cl.SETS:
        out = []
        for cls, (a, b) in jobs:
            an, T, first = cl.rem_align_recorded([a, b], indexmod=refmod, **kw)
            out.append((an, cl.sha(T)))
            if name == "default":
                roots.append(first)
        full[name] = out
        print("%-9s %6d anchors" % (name, sum(len(r[0]) for r in out)), file=sys.stderr)
    an, T, _ = cl.rem_align_recorded(list(cl.big_job()), indexmod=refmod, **cl.BIG_SET[1])
    big = dict(anchors=[[l, p[0], p[1]] for l, p in an], sha=cl.sha(T))
    candidates = [cl.root_candidates(pair, 20) for _, pair in jobs]
    big_candidates = cl.root_candidates(cl.big_job(), 20)
    names = [n for n, _ in cl.SETS]
    bad = conditions(cl, jobs, [r[0] for r in full["default"]], {n: [cl.digest(r[0]) for r in full[n]] for n in names[1:]}, roots, candidates, big_candidates,
                     lambda j: mc.oracle_job([s.upper().encode() for s in jobs[j][1]], minl=20)[0])
    for b in bad:
        print(b, file=sys.stderr)
    assert not bad, "the fixture would test nothing"
    results = {}
    for k, name in enumerate(names):
        rows = []
        for j, (an, sha) in enumerate(full[name]):
            same = next((e for e in names[:k] if full[e][j] == (an, sha)), None)
            if same is not None:
                rows.append(dict(same=same))
            else:
                rows.append(dict(anchors=[[l, p[0], p[1]] for l, p in an], sha=sha))
        results[name] = rows
    doc = dict(sets=names, jobs=len(jobs), results=results, big=big, roots=[None if r is None else [r[0], r[1][0], r[1][1]] for r in roots],
               candidates=candidates + [big_candidates])
    with open(cl.GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    size = os.path.getsize(cl.GOLDEN)
    print("wrote %s (%d bytes)" % (cl.GOLDEN, size), file=sys.stderr)
    assert size < 300 * 1000, "the fixture is larger than 300 KB"


if __name__ == "__main__":
    main()
