#!/usr/bin/env python3
"""Writes tests/golden/many_chain_limits.json: what `reveal refine --method reveal_rem` computes for the jobs of tests/many_chain_limits_cases.py -- `rem.align`
with the reference's default picker (schemes.graphmumpicker) per job, on the REFERENCE's own index module (oracle/_ref/reveallib.so: `make -C oracle && make
-C oracle refmod`), under the eight weight sets of every class (weights at the class' bound W, and W + 1), exactly as the five sibling generators do.  Per
class, job and set: the sorted anchors [l, member, ..] with the members in the order graphalign got them, in the coordinates of the job's text `s0$s1$..`,
and the SHA-256 of the final text; a result an earlier set already has is kept once ("same").  Also, from watching schemes.chain, under "extremes" per
class: the largest |score| of any returned chain and the largest product wpen x gapcost between consecutive chain members per set ("score", "penalty"),
and the largest position of any anchor relative to its sequence's begin, over every set, per job and sequence index ("job_positions") and per sequence
index over the class ("positions").  The sequences are not stored.  CPU only (the host library is needed for rv_chain, which schemes.chain calls).

It refuses to write a fixture that tests nothing (conditions; tests/test_cpu_many_chain_limits.py checks them again from the file):
  (a) `wmax` and `over` equal `default` job for job: scores scale linearly with a common weight, so a difference is a generator bug;
  (b) `pen-max` changes at least 3 jobs of every class against `default`;
  (c) `score-max` changes at least 5 jobs in all, and at least one in each of three classes;
  (d) under `wmax` or `pen-max` the largest |score| of a class reaches 2^26 (chain), 2^22 (chain_multi: 2048 ranks cap it), 2^24 (chain_wide), 2^26
      (chain_large), 2^29 (chain_large_multi), and the largest penalty product of chain_large_multi 2^28;
  (e) positions relative to the sequence's begin: in chain_large an anchor at 2^16 or beyond on path 0 in one job and on path 1 in another; in
      chain_large_multi one in sample 0 and one in the last sample of a job of 16 sequences; in chain_multi and chain_wide one at 1024 or beyond in the
      last sample.
The file stays below 256 KB."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

MAX_BYTES = 256 * 1000
SCORE_MIN = dict(chain=1 << 26, chain_multi=1 << 22, chain_wide=1 << 24, chain_large=1 << 26, chain_large_multi=1 << 29)
PENALTY_MIN = dict(chain_large_multi=1 << 28)


def conditions(lm, results, extremes):
    """conditions (a) - (e) on a fixture: results = {class: {set: [(sorted anchors, sha) per job]}}, extremes as the file keeps them -> list of failures"""
    bad = []
    changed_by_score = {}
    for cls in lm.CLASSES:
        res = results[cls]
        n = len(res["default"])
        for name in ("wmax", "over"):
            differ = [j for j in range(n) if res[name][j] != res["default"][j]]
            if differ:
                bad.append("(a) %s: set %s differs from default on jobs %r" % (cls, name, differ))
        changed = sum(res["pen-max"][j] != res["default"][j] for j in range(n))
        if changed < 3:
            bad.append("(b) %s: pen-max changes only %d jobs" % (cls, changed))
        changed_by_score[cls] = sum(res["score-max"][j] != res["default"][j] for j in range(n))
        ext = extremes[cls]
        score = max(ext["score"]["wmax"], ext["score"]["pen-max"])
        if score < SCORE_MIN[cls]:
            bad.append("(d) %s: the largest |score| is %d, below %d" % (cls, score, SCORE_MIN[cls]))
        pen = max(ext["penalty"]["wmax"], ext["penalty"]["pen-max"])
        if pen < PENALTY_MIN.get(cls, 0):
            bad.append("(d) %s: the largest penalty product is %d, below %d" % (cls, pen, PENALTY_MIN[cls]))
        if ext["positions"] != [max([p[q] for p in ext["job_positions"] if q < len(p)]) for q in range(max(map(len, ext["job_positions"])))]:
            bad.append("(e) %s: positions is not the maximum of job_positions" % cls)
    if sum(changed_by_score.values()) < 5 or sum(1 for v in changed_by_score.values() if v) < 3:
        bad.append("(c) score-max changes %r" % changed_by_score)
    pos = {cls: extremes[cls]["job_positions"] for cls in lm.CLASSES}
    for path in (0, 1):
        if not any(p[path] >= 1 << 16 for p in pos["chain_large"]):
            bad.append("(e) chain_large: no anchor at 2^16 or beyond on path %d" % path)
    if len({next((j for j, p in enumerate(pos["chain_large"]) if p[path] >= 1 << 16), None) for path in (0, 1)}) < 2:
        bad.append("(e) chain_large: the two paths reach 2^16 in one job only")
    if not any(p[0] >= 1 << 16 for p in pos["chain_large_multi"]):
        bad.append("(e) chain_large_multi: no anchor at 2^16 or beyond in sample 0")
    if not any(len(p) == 16 and p[15] >= 1 << 16 for p in pos["chain_large_multi"]):
        bad.append("(e) chain_large_multi: no anchor at 2^16 or beyond in the last sample of a job of 16 sequences")
    for cls in ("chain_multi", "chain_wide"):
        if not any(p[-1] >= 1024 for p in pos[cls]):
            bad.append("(e) %s: no anchor at 1024 or beyond in the last sample" % cls)
    return bad


def run_class(lm, cls, refmod, log=None):
    """-> ({set: [(sorted anchors, sha) per job]}, extremes of the class)"""
    jobs = lm.jobs(cls)
    res, score, penalty = {}, {}, {}
    top = [[-1] * len(seqs) for _, seqs in jobs]
    for x, name in enumerate(lm.SET_NAMES):
        ext = dict(score=0, penalty=0)
        out = []
        for j, (_, seqs) in enumerate(jobs):
            kw = lm.sets(cls, big=lm.is_big(cls, j))[x][1]
            an, T = lm.rem_align_recorded(seqs, ext, indexmod=refmod, **kw)
            out.append((an, lm.sha(T)))
            top[j] = [max(a, b) for a, b in zip(top[j], lm.relative_positions(seqs, an))]
            if cls in lm.LARGE_CLASSES and j < len(lm.fillers(cls)):
                # a filler rides in the call of the jobs of 2^17 ranks, under that call's seedsize and maxmums: they change nothing for it
                an2, T2 = lm.rem_align_job(seqs, indexmod=refmod, **lm.sets(cls, big=True)[x][1])
                assert (an2, lm.sha(T2)) == out[-1], "filler %d of %s depends on seedsize / maxmums under %s" % (j, cls, name)
        res[name], score[name], penalty[name] = out, ext["score"], ext["penalty"]
        if log:
            print("%-18s %-11s %5d anchors, |score| <= %d, penalty <= %d" % (cls, name, sum(len(r[0]) for r in out), ext["score"], ext["penalty"]), file=log)
    positions = [max(p[q] for p in top if q < len(p)) for q in range(max(map(len, top)))]
    return res, dict(score=score, penalty=penalty, positions=positions, job_positions=top)


def main():
    import many_chain_limits_cases as lm
    import pin_oracle
    refmod = pin_oracle.load_refmod(False)
    if refmod is None:
        sys.exit("oracle/_ref/reveallib.so is not built: make -C oracle && make -C oracle refmod")
    full, extremes = {}, {}
    for cls in lm.CLASSES:
        full[cls], extremes[cls] = run_class(lm, cls, refmod, log=sys.stderr)
    bad = conditions(lm, full, extremes)
    for b in bad:
        print(b, file=sys.stderr)
    assert not bad, "the fixture would test nothing"
    results = {}
    for cls in lm.CLASSES:
        results[cls] = {}
        for x, name in enumerate(lm.SET_NAMES):
            rows = []
            for j, (an, sha) in enumerate(full[cls][name]):
                same = next((e for e in lm.SET_NAMES[:x] if full[cls][e][j] == (an, sha)), None)
                rows.append(dict(same=same) if same is not None else dict(anchors=[[l] + list(p) for l, p in an], sha=sha))
            results[cls][name] = rows
    doc = dict(sets=list(lm.SET_NAMES), classes=list(lm.CLASSES), jobs={cls: len(lm.jobs(cls)) for cls in lm.CLASSES}, results=results, extremes=extremes)
    text = json.dumps(doc, separators=(",", ":")) + "\n"
    assert len(text) < MAX_BYTES, "the fixture would have %d bytes" % len(text)
    with open(lm.GOLDEN, "w") as f:
        f.write(text)
    print("wrote %s (%d bytes)" % (lm.GOLDEN, len(text)), file=sys.stderr)


if __name__ == "__main__":
    main()
