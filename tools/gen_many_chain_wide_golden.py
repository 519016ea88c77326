#!/usr/bin/env python3
"""Writes tests/golden/many_chain_wide.json: what `reveal refine --method reveal_rem` computes for the jobs of tests/many_chain_wide_cases.py -- `rem.align`
with the reference's default picker (schemes.graphmumpicker) per job of 17 .. 64 sequences, on the REFERENCE's own index module (oracle/_ref/reveallib.so:
`make -C oracle && make -C oracle refmod`), under every parameter set of the cases module.  Per job and set: the sorted anchors as [l, member, ..] with
the members in the order graphalign got them, in the coordinates of the job's text `s0$s1$..`, and the SHA-256 of the final text; for the sets of
many_chain_wide_cases.HASHED_SETS the anchor count and a SHA-256 of the anchor list instead (an anchor of such a job has up to 64 members), and for
every set a reference to an earlier set of the list where that set has the same result for the job (the file would have 334 484 bytes with
every result written out, against a limit of 294 912).  The sequences
are not stored: the cases module regenerates them.  CPU only (the host library is needed for rv_chain, which schemes.chain calls).

It refuses to write a fixture that tests nothing (fixture_conditions; tests/test_cpu_many_chain_wide.py checks them again from the file):
  (a) no job raises in the reference under any set
  (b) under the default set at least half of the jobs reach `segment` or carry an anchor on a proper subset of their samples
  (c) under the default set at least half of the jobs differ from the built-in picker's anchors (many_multi_cases.oracle_job)
  (d) every weight or gap-model set changes at least 5 jobs against minl5, at least one of them a job of 33 or more sequences
  (e) every k of many_wide_cases.K_VALUES occurs
  (f) star-avg and star-med each change at least 5 jobs against wpen0 (no penalty at all) and differ from each other on at least 5, in each case with a
      job of 33 or more sequences among them: a star gap cost that only switched the penalty off, or one model's value for the other, would show"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

MAX_BYTES = 288 * 1024      # the largest golden JSON of the repository when this fixture was added: stay below it


def main():
    import many_chain_wide_cases as cw
    import pin_oracle
    from gen_many_chain_multi_golden import run_job
    refmod = pin_oracle.load_refmod(False)
    if refmod is None:
        sys.exit("oracle/_ref/reveallib.so is not built: make -C oracle && make -C oracle refmod")
    jobs = cw.jobs()
    results, reach, raised = {}, {}, {}
    for name, kw in cw.SETS:
        out, reach[name], raised[name] = [], [], []
        for cls, seqs in jobs:
            count = dict(segment=0, raised=0)
            an, T = run_job(cw, seqs, refmod, kw, count)
            out.append(cw.record(name, an, T))
            reach[name].append(count["segment"]); raised[name].append(count["raised"])
        results[name] = out
        print("%-9s %6d anchors, %3d jobs reach segment, %d jobs raise" % (name, sum(r["n"] if "n" in r else len(r["anchors"]) for r in out),
                                                                           sum(1 for c in reach[name] if c), sum(1 for c in raised[name] if c)), file=sys.stderr)
    # most jobs do not depend on the weights, the gap model or minn: a result that an earlier set of the list has for the job is kept once
    names = [n for n, _ in cw.SETS]
    full = {n: list(results[n]) for n in names}
    for x, name in enumerate(names):
        for j in range(len(jobs)):
            first = next((e for e in names[:x] if full[e][j] == full[name][j]), None)
            if first is not None:
                results[name][j] = dict(same_as=first)
    doc = dict(sets=[n for n, _ in cw.SETS], jobs=len(jobs), results=results, segment=reach["default"], raised={n: sum(1 for c in raised[n] if c) for n in raised})
    for line in fixture_conditions(cw, jobs, doc):
        print(line, file=sys.stderr)
    for name in doc["sets"]:
        print("%-9s %d bytes" % (name, len(json.dumps(results[name], separators=(",", ":")))), file=sys.stderr)
    text = json.dumps(doc, separators=(",", ":")) + "\n"
    assert len(text) < MAX_BYTES, "the fixture would have %d bytes" % len(text)
    with open(cw.GOLDEN, "w") as f:
        f.write(text)
    print("wrote %s (%d bytes)" % (cw.GOLDEN, os.path.getsize(cw.GOLDEN)), file=sys.stderr)


def fixture_conditions(cw, jobs, doc):
    """asserts (a) - (e) on the document (as written, or as read back from the file) -> the lines of a report"""
    import many_multi_cases as mm
    import many_wide_cases as mw
    res = cw.resolve(doc["results"])
    lines, bad = [], []
    assert sorted(doc["raised"]) == sorted(doc["sets"]) and all(v == 0 for v in doc["raised"].values()), "(a) jobs raise in the reference: %r" % doc["raised"]
    lines.append("(a) no job raises under any of the %d sets" % len(doc["sets"]))
    anchors = lambda r: [(a[0], tuple(a[1:])) for a in r["anchors"]]
    subset = differ = 0
    for j, (cls, seqs) in enumerate(jobs):
        sets = cw.sample_sets(seqs, anchors(res["default"][j]))
        subset += bool(doc["segment"][j]) or any(len(s) < len(seqs) for s in sets)
        want, _ = mm.oracle_job([s.upper().encode() for s in seqs], 20)
        differ += [(l, tuple(sorted(p))) for l, p in anchors(res["default"][j])] != [(l, tuple(p)) for l, p in want]
    lines.append("(b) jobs that reach segment or anchor a proper sample subset: %d of %d" % (subset, len(jobs)))
    assert 2 * subset >= len(jobs), "(b) " + lines[-1]
    lines.append("(c) jobs whose anchors differ from the built-in picker's: %d of %d" % (differ, len(jobs)))
    assert 2 * differ >= len(jobs), "(c) " + lines[-1]
    key = lambda r: r["anchors"] if "anchors" in r else (r["n"], r["asha"])
    for name in cw.WEIGHT_SETS:
        changed = [j for j in range(len(jobs)) if key(res[name][j]) != key(res["minl5"][j])]
        wide = sorted({len(jobs[j][1]) for j in changed if len(jobs[j][1]) >= 33})
        lines.append("(d) %-9s changes %d jobs against minl5, k >= 33 among them: %s" % (name, len(changed), wide or "none"))
        if len(changed) < 5 or not wide: bad.append(lines[-1])
    assert not bad, "\n".join(lines)
    for a, b in (("star-avg", "wpen0"), ("star-med", "wpen0"), ("star-avg", "star-med")):
        changed = [j for j in range(len(jobs)) if key(res[a][j]) != key(res[b][j])]
        wide = sorted({len(jobs[j][1]) for j in changed if len(jobs[j][1]) >= 33})
        lines.append("(f) %-9s differs from %-8s on %d jobs, k >= 33 among them: %s" % (a, b, len(changed), wide or "none"))
        assert len(changed) >= 5 and wide, "\n".join(lines)
    ks = sorted({len(seqs) for _, seqs in jobs})
    lines.append("(e) k of the jobs: %s" % ks)
    assert all(k in ks for k in mw.K_VALUES), "(e) " + lines[-1]
    return lines


if __name__ == "__main__":
    main()
