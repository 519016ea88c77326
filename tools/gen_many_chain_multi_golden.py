#!/usr/bin/env python3
"""Writes tests/golden/many_chain_multi.json: what `reveal refine --method reveal_rem` computes for the jobs of tests/many_chain_multi_cases.py -- `rem.align`
with the reference's default picker (schemes.graphmumpicker) per job, on the REFERENCE's own index module (oracle/_ref/reveallib.so: `make -C oracle &&
make -C oracle refmod`), under every parameter set of the cases module.  Per job and set: the sorted anchors as [l, member, ..] with the members in the
order graphalign got them, in the coordinates of the job's text `s0$s1$..`, and the SHA-256 of the final text.  The sequences are not stored: the cases
module regenerates them.  CPU only (the host library is needed for rv_chain, which schemes.chain calls).

It refuses to write a fixture that tests nothing (fixture_conditions; tests/test_cpu_many_chain_multi.py checks them again from the file):
  (a) no job raises in the reference (trim_overlap's IndexError, segment's KeyError)
  (b) under the default set at least half of the jobs reach `segment` or carry an anchor on a proper subset of their samples
  (c) under the default set at least half of the jobs differ from the built-in picker's anchors (many_cases.oracle_job)
  (d) every other set changes at least 10 jobs against the default set"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def run_job(cm, seqs, refmod, kw, count):
    """rem.align on one job with the picker wrapped: counts the calls that reach `segment` and the calls that raise"""
    from reveal_amd import schemes
    orig = schemes.GraphPicker.graphmumpicker

    def wrapped(self, mums, idx, precomputed=False, minlength=0):
        if not precomputed and len(mums) and idx.nsamples > 2 and not any(m[1] == idx.nsamples for m in mums):
            count["segment"] += 1
        before = count["raised"]
        try:
            r = orig(self, mums, idx, precomputed, minlength)
        except Exception:
            count["raised"] = before + 1
            raise
        return r
    schemes.GraphPicker.graphmumpicker = wrapped
    try:
        return cm.rem_align_job(seqs, indexmod=refmod, **kw)
    except Exception as e:      # (whatever the run makes of a picker that raised: the job counts under (a))
        count["raised"] += 1
        print("a job raised: %r" % (e,), file=sys.stderr)
        return [], ""
    finally:
        schemes.GraphPicker.graphmumpicker = orig


def main():
    import many_chain_multi_cases as cm
    import pin_oracle
    refmod = pin_oracle.load_refmod(False)
    if refmod is None:
        sys.exit("oracle/_ref/reveallib.so is not built: make -C oracle && make -C oracle refmod")
    jobs = cm.jobs()
    results, reach, raised = {}, {}, {}
    for name, kw in cm.SETS:
        out, reach[name], raised[name] = [], [], []
        for cls, seqs in jobs:
            count = dict(segment=0, raised=0)
            an, T = run_job(cm, seqs, refmod, kw, count)
            out.append(dict(anchors=[[l] + list(p) for l, p in an], sha=cm.sha(T)))
            reach[name].append(count["segment"]); raised[name].append(count["raised"])
        results[name] = out
        print("%-9s %6d anchors, %3d jobs reach segment, %d jobs raise" % (name, sum(len(r["anchors"]) for r in out), sum(1 for c in reach[name] if c),
                                                                           sum(1 for c in raised[name] if c)), file=sys.stderr)
    doc = dict(sets=[n for n, _ in cm.SETS], jobs=len(jobs), results=results, segment=reach["default"], raised={n: sum(1 for c in raised[n] if c) for n in raised})
    for line in fixture_conditions(cm, jobs, doc):
        print(line, file=sys.stderr)
    with open(cm.GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (cm.GOLDEN, os.path.getsize(cm.GOLDEN)), file=sys.stderr)


def fixture_conditions(cm, jobs, doc):
    """asserts (a) - (d) on the document (as written, or as read back from the file) -> the lines of a report"""
    import many_cases as mc
    res = doc["results"]
    lines, bad = [], []
    assert all(v == 0 for v in doc["raised"].values()), "(a) jobs raise in the reference: %r" % doc["raised"]
    anchors = lambda r: [(a[0], tuple(a[1:])) for a in r["anchors"]]
    subset = differ = 0
    for j, (cls, seqs) in enumerate(jobs):
        sets = cm.sample_sets(seqs, anchors(res["default"][j]))
        subset += bool(doc["segment"][j]) or any(len(s) < len(seqs) for s in sets)
        want, _ = mc.oracle_job([s.upper().encode() for s in seqs], minl=20)
        differ += [(l, tuple(sorted(p))) for l, p in anchors(res["default"][j])] != [(l, tuple(p)) for l, p in want]
    lines.append("(b) jobs that reach segment or anchor a proper sample subset: %d of %d" % (subset, len(jobs)))
    assert 2 * subset >= len(jobs), "(b) " + lines[-1]
    lines.append("(c) jobs whose anchors differ from the built-in picker's: %d of %d" % (differ, len(jobs)))
    assert 2 * differ >= len(jobs), "(c) " + lines[-1]
    for name in doc["sets"][1:]:
        changed = sum(res[name][j]["anchors"] != res["default"][j]["anchors"] for j in range(len(jobs)))
        lines.append("(d) %-9s changes %d jobs against the default set" % (name, changed))
        if changed < 10: bad.append(lines[-1])
    assert not bad, "\n".join(lines)
    return lines


if __name__ == "__main__":
    main()
