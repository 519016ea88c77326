"""inputs of the align_many tests with the reference's default picker for pair jobs above 2048 ranks (RV_MANY_CHAIN_LARGE; tests/test_cpu_many_chain_large.py
checks the list and the golden file, tests/test_gpu_many_chain_large.py runs it): the large class jobs of many_large_cases, a class of its own whose alleles
carry swapped, dropped or duplicated blocks of a few hundred bases -- where trimming and chaining choose other anchors than the longest match --, a class of
long alleles 1 % apart with more than 64 matches at the root, and the corners: the first size above the leaf kernel's, alleles of 9 999 bases (1 % apart,
and identical), and one job of 80 002 ranks (2 x 40 000 bases) whose TEXT positions do not fit 16 bits -- the positions k_pick_chain packs are relative
to the interval begins and stay below 40 000 there, bit 16 of neither field is set; tests/many_chain_limits_cases.py has the jobs of 2^17 ranks that set
it on either path (tests/test_gpu_many_chain_limits.py test_the_jobs_of_2_17_ranks).  Deterministic.  The expected results (tests/golden/many_chain_large.json,
written by tools/gen_many_chain_large_golden.py) come from `rem.align` on the REFERENCE's own index module."""
import hashlib
import json
import os
import random

import many_cases as mc
import many_chain_cases as cc
import many_large_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "many_chain_large.json")

# (name, keyword arguments of rem.align); what is not named: wpen 1, wscore 1, sumofpairs, trim, seedsize 10000, maxmums 10000
SETS = tuple((n, kw) for n, kw in cc.SETS if n != "minl1")
# the job of 80 002 ranks runs under a set of its own: its sequences are longer than rem.align's default seedsize and maxmums, which would not admit it
BIG_SET = ("big", dict(minlength=20, seedsize=100000, maxmums=100000))
N_CLASS = 20
N_REARRANGED = 30
N_DIVERGENT = 4
REARRANGED_RANKS = (2100, 9000)


def rearranged_large(rng):
    """6 .. 14 blocks of 150 .. 600 bases; the second allele has two blocks swapped, one dropped or duplicated, 1 % substitutions; 2100 .. 9000 ranks"""
    while True:
        nb = rng.randint(6, 14)
        blocks = [mc.rnd(rng, rng.randint(150, 600)) for _ in range(nb)]
        order = list(range(nb)); i, j = rng.sample(range(nb), 2); order[i], order[j] = order[j], order[i]
        if rng.random() < 0.5:
            order.pop(rng.randrange(len(order)))
        else:
            k = rng.randrange(nb); order.insert(rng.randrange(len(order) + 1), k)
        a = "".join(blocks); b = "".join(mc.mutate(rng, blocks[k], 0.01) for k in order)
        if REARRANGED_RANKS[0] <= len(a) + len(b) + 2 <= REARRANGED_RANKS[1]:
            return a, b


def divergent_large(rng):
    """alleles of 8 500 .. 9 999 bases, 1 % apart: about 80 matches of 20 and more bases at the root"""
    a = mc.rnd(rng, rng.randint(8500, 9999))
    return a, mc.mutate(rng, a, 0.01)


def corner_jobs():
    """-> [(class, (a, b))]: 2049 ranks; 2 x 9 999 bases 1 % apart; 2 x 9 999 identical (many_large_cases.corner_jobs' own)"""
    c = lc.corner_jobs()
    assert [len(a) + len(b) + 2 for a, b in c] == list(lc.CORNER_RANKS)
    return [("first-large", c[0]), ("allele-10k", c[5]), ("allele-10k-identical", c[6])]


def big_job():
    """the job of 80 002 ranks (text positions beyond 16 bits; the kernel's positions, relative to the interval begins, stay below 2^16)"""
    a, b = lc.corner_jobs()[7]
    assert len(a) + len(b) + 2 == 80002
    return a, b


def fillers():
    """three small jobs that bring the call with the job of 80 002 ranks up to RV_MANY_CHAIN_LARGE_MIN admitted jobs"""
    return [pair for _, pair in lc.large_class_jobs(1)[:3]]


def jobs():
    """-> [(class, (a, b))]: many_large_cases.large_class_jobs(2), 30 `rearranged-large` jobs, 4 `divergent-large` jobs, the three corners"""
    out = list(lc.large_class_jobs(2))
    rng = random.Random(79)
    out += [("rearranged-large", rearranged_large(rng)) for _ in range(N_REARRANGED)]
    rng = random.Random(80)
    out += [("divergent-large", divergent_large(rng)) for _ in range(N_DIVERGENT)]
    return out + corner_jobs()


picker_args = cc.picker_args
sha = cc.sha


def rem_align_recorded(seqs, indexmod=None, **kw):
    """cc.rem_align_job that also keeps the order of the picks -> (sorted anchors, final text, first pick (l, (pa, pb)) or None)"""
    from reveal_amd import rem
    rec = []

    class Rec(rem.GraphAligner):
        def graphalign(self, index, mum):
            rec.append((int(mum[0]), tuple(sorted(int(p) for _, p in mum[2]))))
            return super().graphalign(index, mum)
    orig = rem.GraphAligner
    rem.GraphAligner = Rec
    try:
        G, idx = rem.align([("s%d" % k, s) for k, s in enumerate(seqs)], indexmod=indexmod, **kw)
    finally:
        rem.GraphAligner = orig
    T = idx.T
    return sorted(rec), (T if isinstance(T, str) else T.decode("latin-1")), (rec[0] if rec else None)


def root_candidates(pair, minl):
    """the matches the recursion's scan finds at the root of the job (CPU oracle, reveal.c:119-180)"""
    from helpers import assemble, oracle
    T, nsep, nodes = assemble([s.upper().encode() for s in pair], toupper=False)
    O = oracle(False)
    c = O.construct(T, nsep, 2)
    return len(O.getmums(c["tbuf"], c["SA"], c["LCP"], c["nsep"], minl, rem=True)[0])


def children_ranks(pair, pick):
    """ranks of the leading and the trailing child of the root after the split on `pick` (l, (pa, pb)), positions of the text a$b$"""
    la, lb = len(pair[0]), len(pair[1])
    l, (pa, pb) = pick
    pb -= la + 1
    return pa + pb, (la - pa - l) + (lb - pb - l)


def digest(anchors):
    return hashlib.sha256(json.dumps([[l, p[0], p[1]] for l, p in anchors], separators=(",", ":")).encode()).hexdigest()


def load_golden():
    """-> {set name: [(sorted anchors [(l, (pa, pb))], sha256 of the final text)] in the order of jobs()}, "big": the one entry of the job of 80 002 ranks,
    "roots": the first pick of every job under `default`, "candidates": matches at every job's root and, last, at the big job's (minl 20).
    The file keeps a result an earlier set already has only once ("same")."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["sets"] == [n for n, _ in SETS] and doc["jobs"] == len(jobs())
    out = {}

    def entry(r):
        return ([(a[0], (a[1], a[2])) for a in r["anchors"]], r["sha"])
    for n, _ in SETS:
        out[n] = [out[r["same"]][j] if "same" in r else entry(r) for j, r in enumerate(doc["results"][n])]
    out["big"] = [entry(doc["big"])]
    out["roots"] = [None if r is None else (r[0], (r[1], r[2])) for r in doc["roots"]]
    out["candidates"] = doc["candidates"]
    return out
