#!/usr/bin/env python3
"""The pick stage of k_leaf_multi_chain (csrc/rv_leaf_multi_chain.hip) restated as a Python picker callback and run inside `rem.align` on the REFERENCE's
own index module, over every job and parameter set of tests/many_chain_multi_cases.py.  It has to reproduce tests/golden/many_chain_multi.json, which the
reference's own graphmumpicker wrote.  What it pins before any kernel runs: the list order `segment` breaks its tie by (first-seen group, strict >),
trim per member index with the stable (position, -l) order, the chain's tie order as ONE key (candidate score, predecessor's score, step of activation,
sort order) without the `active` list, the entry of rv_chain's dictionaries that matches with one place on the first path share (`shared` counts the
chains where that happens), and how often the kernel's give-ups would fire (1: trim_overlap raises, 2: no predecessor, 8: another match carries the
split's offsets) -- a call that gives up falls back to the reference's picker here, as a flagged job reruns the ordinary way.  The scan's order is
pinned separately (many_chain_multi_cases.kernel_scan, tests/test_cpu_many_chain_multi.py).  CPU only.  Prints per set: jobs equal to the golden file,
picker calls, calls per give-up.

`--cases wide`: the same over tests/many_chain_wide_cases.py and tests/golden/many_chain_wide.json -- jobs of 17 .. 64 sequences, the 64-sample form of
the kernel.  That form holds ONE predecessor of a chain step per wavefront where the 16-sample form holds four; the predecessors are still taken by
ascending sort order, the step of activation is the match at which a predecessor first ends in front, and the choice is the maximum of the one key,
whatever the order the candidates are looked at in.  What it does differently is the gap cost over up to 64 paths, and `gapcost_lanes` restates that
arithmetic lane by lane -- a lane per sample, the set's paths taken in turn, two sums per lane, wave sums with the lanes outside the set contributing
zero -- and is what the picker uses under `--cases wide` (tests/test_cpu_many_chain_wide.py also holds it against `gapcost` on random gaps with ties).

`--cases wide_large`: the same over tests/many_chain_wide_large_cases.py and tests/golden/many_chain_wide_large.json -- jobs of 17 .. 64 sequences above
2048 ranks, the 64-sample form of k_pick_multi_chain (csrc/rv_pick_multi_chain.hip).  Its chain step is the 64-lane one (`gapcost_lanes`); what it adds
is restated here as well: the sample of a member by binary search over the ascending begins of the sub-index' live intervals, a coordinate as position
(17 bits) | sample << 17 (six bits) whose order is the order of the text, sample sets as 64-bit words, and the cap of 256 candidates -- the matches in
every sample, all of the list where there is none -- above which the kernel flags the job (give-up 32).  The job whose positions need 17 bits runs too,
under its own set."""
import argparse
import bisect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

GCMODEL = {"sumofpairs": 0, "star-avg": 1, "star-med": 2}


def gapcost(d, model):
    k = len(d)
    if model == 1:
        return abs(sum(d)) // k
    D = [abs(x) for x in d]
    if model == 2:
        return sorted(D)[k // 2]
    return sum(abs(D[i] - D[j]) for i in range(k) for j in range(i + 1, k))


def gapcost_lanes(d_by_sample, model, lanes=64):
    """the gap cost as the 64-sample form of the kernel computes it: d_by_sample = {sample: d} over the set's paths.  Lane s holds d of sample s (0
    outside the set) and D = |d|; for every path j of the set in ascending order the lane reads D[j] (readlane) and, if it is in the set itself, adds
    |D - D[j]| for j above it (its share of the pairs) and counts the D[j] below its own, ties by lane (its rank).  star-avg: |wave sum of d| / k with C's
    truncation; star-med: wave sum of D over the lanes whose rank is k / 2 (exactly one); sum of pairs: wave sum of the shares"""
    inset = [s in d_by_sample for s in range(lanes)]
    d = [d_by_sample.get(s, 0) for s in range(lanes)]
    D = [abs(x) for x in d]
    k = sum(inset)
    acc, rank = [0] * lanes, [0] * lanes
    if model != 1:
        for j in (s for s in range(lanes) if inset[s]):
            od = D[j]
            for lane in range(lanes):
                if inset[lane]:
                    if j > lane:
                        acc[lane] += abs(D[lane] - od)
                    rank[lane] += 1 if (od < D[lane] or (od == D[lane] and j < lane)) else 0
    if model == 1:
        return int(abs(sum(d)) / k)
    if model == 2:
        return sum(D[lane] if inset[lane] and rank[lane] == k // 2 else 0 for lane in range(lanes))
    return sum(acc)


POS_BITS, WIDE_CAP = 17, 256      # MultiPickStage<64>: bits of a position inside its interval; RV_PICK_WCHAIN_CAP_MAX


def make_picker(seqs, args, stat, orig, wide=False, large=False):
    ends, at = [], 0
    for s in seqs:
        at += len(s) + 1
        ends.append(at)
    begins = [0] + ends[:-1]

    def sample_of(p):
        return next(q for q, e in enumerate(ends) if p < e)

    def give_up(self, bit, mums, idx, minlength):
        stat[bit] = stat.get(bit, 0) + 1
        return orig(self, mums, idx, False, minlength)

    def picker(self, mums, idx, precomputed=False, minlength=0):
        assert not precomputed
        stat["calls"] = stat.get("calls", 0) + 1
        if len(mums) == 0:
            return ()
        iv = {sample_of(b): (b, e) for b, e in (tuple(x) for x in idx.nodes)}
        ns = idx.nsamples
        cand = [[m[0], [p for _, p in m[2]], 0] for m in mums]               # l, members in the order handed out, shift
        if large:
            # the 64-sample form of k_pick_multi_chain: what counts against the cap, the sample of a member by binary search over the live begins, the
            # packed coordinate and the 64-bit sample set
            full = sum(1 for c in cand if len(c[1]) == ns)
            if (full if full else len(cand)) > WIDE_CAP:
                return give_up(self, 32, mums, idx, minlength)
            lsmp = sorted(iv, key=lambda s: iv[s][0])
            lbeg = [iv[s][0] for s in lsmp]
            assert lsmp == sorted(lsmp), "the live intervals ascend with their samples: the text is sample-major"

            def packed(p, l):
                s = lsmp[bisect.bisect_right(lbeg, p) - 1]
                assert s == sample_of(p) and iv[s][0] <= p and p + l <= iv[s][1] and s < 64 and p - iv[s][0] < 1 << POS_BITS
                return (s << POS_BITS) | (p - iv[s][0])
            for l, mem, _ in cand:
                crd = [packed(p, l) for p in mem]
                assert [c >> POS_BITS for c in crd] == [sample_of(p) for p in mem]
                assert sorted(range(len(mem)), key=lambda q: crd[q]) == sorted(range(len(mem)), key=lambda q: mem[q])      # the order of the text
                word = 0
                for c in crd:
                    assert not (word >> (c >> POS_BITS)) & 1
                    word |= 1 << (c >> POS_BITS)
                assert word < 1 << 64
        masks = [frozenset(sample_of(p) for p in c[1]) for c in cand]
        if any(len(c[1]) == ns for c in cand):
            want = frozenset(iv)
        elif ns > 2:
            best = None
            for i, mk in enumerate(masks):
                z = sum(cand[j][0] for j in range(len(cand)) if masks[j] == mk) * len(mk)
                key = (z, -masks.index(mk))
                best = key if best is None or key > best else best
            want = masks[-best[1]]
        else:
            return ()
        A = [c for c, mk in zip(cand, masks) if mk == want]
        kset = len(want)
        pos = lambda x, c: x[1][c] + x[2]
        for c in range(kset):
            if len(A) <= 1:
                break
            B = sorted(A, key=lambda x: (pos(x, c), -x[0]))
            end = lambda x: pos(x, c) + x[0]
            A = [x for i, x in enumerate(B) if (i == 0 and end(B[1]) > end(x)) or end(B[i - 1]) < end(x)]
            if len(A) <= 1:
                break
            st = [list(A[0])]
            for mum in A[1:]:
                if not st:
                    return give_up(self, 1, mums, idx, minlength)
                pm = st[-1]
                ov = end(pm) - pos(mum, c)
                if ov > 0:
                    if pm[0] - ov > 0:
                        pm[0] -= ov
                    else:
                        st.pop()
                    if mum[0] - ov > 0:
                        st.append([mum[0] - ov, mum[1], mum[2] + ov])
                else:
                    st.append(list(mum))
            A = st
        if not A:
            return ()
        coord = lambda x: {sample_of(p): p + x[2] for p in x[1]}
        if len(A) == 1:
            split = A[0]
        else:
            s0 = min(want)
            # rv_chain's stable sort by the first path's coordinate over rv_pick_chain's list (ascending l, equal lengths in trim's order)
            B = sorted(A, key=lambda x: (coord(x)[s0], x[0]))
            keys = [coord(x)[s0] for x in B]
            if len(set(keys)) != len(keys):
                stat["shared"] = stat.get("shared", 0) + 1
            C = [coord(x) for x in B]
            m = len(B)
            step, score, link = [None] * m, [0] * m, [None] * m
            order = sorted(want)
            linkR = None
            for e in range(m + 1):
                start = C[e] if e < m else {s: iv[s][1] for s in order}
                l_e, n_e = (B[e][0], len(B[e][1])) if e < m else (0, 0)
                gain = args.wscore * l_e * (n_e * (n_e - 1) // 2)
                best = None
                for p in range(-1, e):
                    endp = {s: iv[s][0] - 1 for s in order} if p < 0 else {s: C[p][s] + B[p][0] for s in order}
                    d = [endp[s] - start[s] for s in order]
                    if any(x > 0 for x in d):
                        continue
                    if p >= 0 and step[p] is None:
                        step[p] = e
                    sc = 0 if p < 0 else score[p]
                    gap = gapcost_lanes(dict(zip(order, d)), GCMODEL[args.gcmodel]) if wide else gapcost(d, GCMODEL[args.gcmodel])
                    tmpw = sc + gain - args.wpen * gap
                    key = (tmpw, sc, -(0 if p < 0 else ((step[p] + 1) << 12) | p))
                    if best is None or key > best[0]:
                        best = (key, p)
                if best is None:
                    return give_up(self, 2, mums, idx, minlength)
                # rv_chain keeps score and link per first-path coordinate: matches that share it share the entry, the last one's values stand, and a
                # link leads to the last match of the predecessor's coordinate
                lk = best[1]
                while 0 <= lk < m - 1 and keys[lk + 1] == keys[lk]:
                    lk += 1
                if e < m:
                    j = e
                    while j >= 0 and keys[j] == keys[e]:
                        score[j], link[j] = best[0][0], lk
                        j -= 1
                else:
                    linkR = lk
            split, c = None, linkR
            while c >= 0:
                if split is None or B[c][0] > split[0]:
                    split = B[c]
                c = link[c]
            if split is None:
                return ()
        rel = lambda x: tuple(p + x[2] - begins[sample_of(p)] for p in x[1])
        if any(x is not split and rel(x) == rel(split) for x in A):
            return give_up(self, 8, mums, idx, minlength)
        return (split[0], len(split[1]), tuple((sample_of(p), p + split[2]) for p in split[1])), [], []
    return picker


def run_wide_large(refmod, sets=None, which=None, big=True, out=None):
    """the prototype over tests/many_chain_wide_large_cases.py: sets (names, default: all), which (job indices, default: all), big (the job whose
    positions need 17 bits, under its own set) -> (jobs that differ from the golden file, give-ups by bit)"""
    import many_chain_wide_large_cases as cw
    from reveal_amd import schemes
    jobs, golden = cw.jobs(), cw.load_golden()
    orig = schemes.GraphPicker.graphmumpicker
    todo = [(name, kw, j, jobs[j][1], golden[name][j]) for name, kw in cw.SETS if sets is None or name in sets
            for j in (range(len(jobs)) if which is None else which)]
    if big:
        todo.append((cw.BIG_SET[0], cw.BIG_SET[1], -1, cw.big_job(), golden["big"][0]))
    bad, gave_up = [], {}
    for name, kw, j, seqs, want in todo:
        stat = {}
        schemes.GraphPicker.graphmumpicker = make_picker([s.upper() for s in seqs], cw.picker_args(kw), stat, orig, wide=True, large=True)
        try:
            an, T = cw.rem_align_job(seqs, indexmod=refmod, **kw)
        finally:
            schemes.GraphPicker.graphmumpicker = orig
        if (an, cw.sha(T)) != want:
            bad.append((name, j))
        for k, v in stat.items():
            if k not in ("calls", "shared"):
                gave_up[k] = gave_up.get(k, 0) + v
        if out:
            print("%-9s job %3d: %s, picker calls %d, gave up: %s" % (name, j, "differs" if (name, j) in bad else "equal", stat.get("calls", 0),
                  {k: v for k, v in stat.items() if k not in ("calls", "shared")} or "never"), file=out)
    return bad, gave_up


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", choices=("multi", "wide", "wide_large"), default="multi",
                    help="multi: jobs of 3 .. 16 sequences (many_chain_multi_cases); wide: 17 .. 64 (many_chain_wide_cases); wide_large: 17 .. 64 above 2048 ranks (many_chain_wide_large_cases)")
    opt = ap.parse_args()
    if opt.cases == "wide_large":
        import pin_oracle
        refmod = pin_oracle.load_refmod(False)
        if refmod is None:
            sys.exit("oracle/_ref/reveallib.so is not built: make -C oracle && make -C oracle refmod")
        bad, gave_up = run_wide_large(refmod, out=sys.stdout)
        print("%d results differ from the golden file; gave up: %s" % (len(bad), gave_up or "never"))
        sys.exit(1 if bad else 0)
    if opt.cases == "wide":
        import many_chain_wide_cases as cm
        matches = lambda rec, an, T: cm.same(rec, an, cm.sha(T))
    else:
        import many_chain_multi_cases as cm
        matches = lambda rec, an, T: (an, cm.sha(T)) == rec
    import pin_oracle
    from reveal_amd import schemes
    refmod = pin_oracle.load_refmod(False)
    if refmod is None:
        sys.exit("oracle/_ref/reveallib.so is not built: make -C oracle && make -C oracle refmod")
    jobs, golden = cm.jobs(), cm.load_golden()
    orig = schemes.GraphPicker.graphmumpicker
    bad = 0
    for name, kw in cm.SETS:
        stat, same = {}, 0
        for j, (cls, seqs) in enumerate(jobs):
            schemes.GraphPicker.graphmumpicker = make_picker([s.upper() for s in seqs], cm.picker_args(kw), stat, orig, wide=opt.cases == "wide")
            try:
                an, T = cm.rem_align_job(seqs, indexmod=refmod, **kw)
            finally:
                schemes.GraphPicker.graphmumpicker = orig
            ok = matches(golden[name][j], an, T)
            same += ok
            if not ok:
                print("  %s job %d (%s) differs" % (name, j, cls))
        bad += len(jobs) - same
        print("%-9s %3d of %3d jobs equal the golden file; picker calls %d, gave up: %s" % (name, same, len(jobs), stat.get("calls", 0),
              {k: v for k, v in stat.items() if k != "calls"} or "never"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
