#!/usr/bin/env python3
"""Writes tests/golden/many_chain_wide_large.json: what `reveal refine --method reveal_rem` computes for the jobs of
tests/many_chain_wide_large_cases.py -- `rem.align` with the reference's default picker (schemes.graphmumpicker) per job, on the REFERENCE's own index
module (oracle/_ref/reveallib.so: `make -C oracle && make -C oracle refmod`), under every parameter set of the cases module, as
tools/gen_many_chain_large_multi_golden.py does for the jobs of 3 .. 16 sequences.  Per job and set: the sorted anchors (l, members in the order
graphalign got them) in the coordinates of the job's text `s0$s1$..` and the SHA-256 of the final text; a result an earlier set already has is kept once
("same").  Also, from watching the picker under `default`: per job the candidates at the root, the samples there, the members of the first pick and
whether `segment` chose the set ("roots"), the most candidates of any sub-index below the root ("below"), and the most candidates of any sub-index of
the job whose positions need 17 bits ("big_most").  The sequences are not stored.  CPU only.

It refuses to write a fixture that tests nothing:
  (a) under `default` at least a third of the `shuffled` / `tied` / `subset` jobs have other anchors than the built-in picker's (many_multi_cases.oracle_job);
  (b) at least 5 jobs whose first pick has fewer members than the job has sequences;
  (c) each of wpen0, star-avg and star-med changes at least 5 jobs against `default`;
  (d) some job holds more than 64 candidates at its root, and some job never more than 8 in any sub-index;
  (e) at least 3 roots go through `segment` (no match in every sample);
  (f) among the jobs each of wpen0, star-avg and star-med changes are jobs of more than 32 sequences;
  (g) no job holds more candidates than the cap of k_pick_multi_chain<64> (256) at its root or below it -- what counts is what the kernel counts: the
      matches in every sample of a sub-index, all of the list where there is none -- and neither does the job whose positions need 17 bits: the tests
      may ask for every job shared.
The file stays below 300 KB."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def conditions(cw, jobs, default, others, roots, below, big_most, builtin_of):
    """the conditions on a fixture: (a) - (e) are gen_many_chain_large_multi_golden.conditions' (the weight sets: its (c)), (f) and (g) as above -> list
    of failures"""
    import gen_many_chain_large_multi_golden as base
    bad = base.conditions(cw, jobs, default, others, roots, below, builtin_of)
    dd = [cw.digest(a) for a in default]
    for name in cw.WEIGHT_SETS:
        wide = sum(others[name][j] != dd[j] and len(jobs[j][1]) > 32 for j in range(len(jobs)))
        if wide < 1:
            bad.append("(f) set %s changes no job of more than 32 sequences" % name)
    over = [j for j, (r, b) in enumerate(zip(roots, below)) if max(r[0], b) > cw.CAP]
    if over:
        bad.append("(g) jobs %r hold more than %d candidates (%r)" % (over, cw.CAP, [max(roots[j][0], below[j]) for j in over]))
    if big_most > cw.CAP:
        bad.append("(g) the job whose positions need 17 bits holds %d candidates in a sub-index" % big_most)
    return bad


def builtin_anchors(cw, seqs):
    import gen_many_chain_large_multi_golden as base
    return base.builtin_anchors(cw, seqs)


def main():
    import many_chain_wide_large_cases as cw
    import pin_oracle
    refmod = pin_oracle.load_refmod(False)
    if refmod is None:
        sys.exit("oracle/_ref/reveallib.so is not built: make -C oracle && make -C oracle refmod")
    jobs = cw.jobs()
    full, roots, below = {}, [], []
    for name, kw in cw.SETS:
        out = []
        for cls, seqs in jobs:
            an, T, calls = cw.rem_align_recorded(seqs, indexmod=refmod, **kw)
            out.append((an, cw.sha(T)))
            if name == "default":
                roots.append([int(x) for x in calls[0]] if calls else [0, len(seqs), 0, 0])
                below.append(max([c[0] for c in calls[1:]] or [0]))
        full[name] = out
        print("%-9s %6d anchors" % (name, sum(len(r[0]) for r in out)), file=sys.stderr)
    print("candidates at the root / below it:", [(r[0], b) for r, b in zip(roots, below)], file=sys.stderr)
    an, T, calls = cw.rem_align_recorded(cw.big_job(), indexmod=refmod, **cw.BIG_SET[1])
    big = dict(anchors=[[l] + list(p) for l, p in an], sha=cw.sha(T))
    big_most = max([c[0] for c in calls] or [0])
    print("big: %d anchors, at most %d candidates" % (len(an), big_most), file=sys.stderr)
    names = [n for n, _ in cw.SETS]
    bad = conditions(cw, jobs, [r[0] for r in full["default"]], {n: [cw.digest(r[0]) for r in full[n]] for n in names[1:]}, roots, below, big_most,
                     lambda j: builtin_anchors(cw, jobs[j][1]))
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
    doc = dict(sets=names, jobs=len(jobs), results=results, big=big, roots=roots, below=below, big_most=big_most)
    with open(cw.GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    size = os.path.getsize(cw.GOLDEN)
    print("wrote %s (%d bytes)" % (cw.GOLDEN, size), file=sys.stderr)
    assert size < 300 * 1000, "the fixture is larger than 300 KB"


if __name__ == "__main__":
    main()
