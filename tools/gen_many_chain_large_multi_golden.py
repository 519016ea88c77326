#!/usr/bin/env python3
"""Writes tests/golden/many_chain_large_multi.json: what `reveal refine --method reveal_rem` computes for the jobs of
tests/many_chain_large_multi_cases.py -- `rem.align` with the reference's default picker (schemes.graphmumpicker) per job, on the REFERENCE's own index
module (oracle/_ref/reveallib.so: `make -C oracle && make -C oracle refmod`), under every parameter set of the cases module, as
tools/gen_many_chain_large_golden.py does for the pair jobs.  Per job and set: the sorted anchors (l, members in the order graphalign got them) in the
coordinates of the job's text `s0$s1$..` and the SHA-256 of the final text; a result an earlier set already has is kept once ("same").  Also, from
watching the picker under `default`: per job the candidates at the root, the samples there, the members of the first pick and whether `segment` chose
the set ("roots"), and the most candidates of any sub-index below the root ("below").  The sequences are not stored.  CPU only.

It refuses to write a fixture that tests nothing:
  (a) under `default` at least a third of the `shuffled` / `tied` / `subset` jobs have other anchors than the built-in picker's (many_multi_cases.oracle_job);
  (b) at least 5 jobs whose first pick has fewer members than the job has sequences;
  (c) each of wpen0, star-avg and star-med changes at least 5 jobs against `default`;
  (d) some job holds more than 64 candidates at its root, and some job never more than 8 in any sub-index;
  (e) at least 3 roots go through `segment` (no match in every sample).
The file stays below 300 KB."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

PICKER_CLASSES = ("shuffled", "tied", "subset")


def conditions(cl, jobs, default, others, roots, below, builtin_of):
    """the five conditions on a fixture: default = [sorted anchors] per job, others = {set: [digest per job]}, roots / below as the file keeps them,
    builtin_of(j) = the built-in picker's sorted anchors of job j (members sorted) -> list of failures"""
    bad = []
    sel = [j for j, (cls, _) in enumerate(jobs) if cls in PICKER_CLASSES]
    differ = sum(builtin_of(j) != sorted((l, tuple(sorted(p))) for l, p in default[j]) for j in sel)
    if 3 * differ < len(sel):
        bad.append("(a) the default picker differs from the built-in one on %d of %d shuffled / tied / subset jobs" % (differ, len(sel)))
    sub = sum(1 for j, r in enumerate(roots) if 0 < r[2] < len(jobs[j][1]))
    if sub < 5:
        bad.append("(b) only %d jobs whose first pick has fewer members than the job has sequences" % sub)
    dd = [cl.digest(a) for a in default]
    for name in cl.WEIGHT_SETS:
        changed = sum(others[name][j] != dd[j] for j in range(len(jobs)))
        if changed < 5:
            bad.append("(c) set %s changes only %d jobs" % (name, changed))
    if not any(r[0] > 64 for r in roots) or not any(max(r[0], b) <= 8 for r, b in zip(roots, below)):
        bad.append("(d) most candidates at a root %d, fewest over a whole job %d" % (max(r[0] for r in roots), min(max(r[0], b) for r, b in zip(roots, below))))
    seg = sum(1 for r in roots if r[3])
    if seg < 3:
        bad.append("(e) only %d roots go through segment" % seg)
    return bad


def builtin_anchors(cl, seqs):
    import many_multi_cases as mm
    return sorted((int(l), tuple(sorted(int(p) for p in pos))) for l, pos in mm.oracle_job([s.upper().encode() for s in seqs], 20)[0])


def main():
    import many_chain_large_multi_cases as cl
    import pin_oracle
    refmod = pin_oracle.load_refmod(False)
    if refmod is None:
        sys.exit("oracle/_ref/reveallib.so is not built: make -C oracle && make -C oracle refmod")
    jobs = cl.jobs()
    full, roots, below = {}, [], []
    for name, kw in cl.SETS:
        out = []
        for cls, seqs in jobs:
            an, T, calls = cl.rem_align_recorded(seqs, indexmod=refmod, **kw)
            out.append((an, cl.sha(T)))
            if name == "default":
                roots.append([int(x) for x in calls[0]] if calls else [0, len(seqs), 0, 0])
                below.append(max([c[0] for c in calls[1:]] or [0]))
        full[name] = out
        print("%-9s %6d anchors" % (name, sum(len(r[0]) for r in out)), file=sys.stderr)
    an, T, _ = cl.rem_align_recorded(cl.big_job(), indexmod=refmod, **cl.BIG_SET[1])
    big = dict(anchors=[[l] + list(p) for l, p in an], sha=cl.sha(T))
    names = [n for n, _ in cl.SETS]
    bad = conditions(cl, jobs, [r[0] for r in full["default"]], {n: [cl.digest(r[0]) for r in full[n]] for n in names[1:]}, roots, below,
                     lambda j: builtin_anchors(cl, jobs[j][1]))
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
                rows.append(dict(anchors=[[l] + list(p) for l, p in an], sha=sha))
        results[name] = rows
    doc = dict(sets=names, jobs=len(jobs), results=results, big=big, roots=roots, below=below)
    with open(cl.GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    size = os.path.getsize(cl.GOLDEN)
    print("wrote %s (%d bytes)" % (cl.GOLDEN, size), file=sys.stderr)
    assert size < 300 * 1000, "the fixture is larger than 300 KB"


if __name__ == "__main__":
    main()
