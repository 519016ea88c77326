"""inputs of the align_many tests that take the five device pickers to the bounds they admit a job up to (tests/test_cpu_many_chain_limits.py checks the
list and the golden file, tests/test_gpu_many_chain_limits.py runs it): per class -- `chain` (pairs up to 2048 ranks, k_leaf_chain), `chain_multi` (3 .. 16
sequences, k_leaf_multi_chain<16>), `chain_wide` (17 .. 64, k_leaf_multi_chain<64>), `chain_large` (pairs above 2048 ranks, k_pick_chain) and
`chain_large_multi` (3 .. 16 sequences above 2048 ranks, k_pick_multi_chain) -- ten to sixteen jobs, run under weight sets at the class' own weight
bound W: (W, W), (1, W), (W, 1), (W, 0), (W, W) under the two star models, and (W + 1, W + 1), which no class admits.

`far` jobs: all members share three to five blocks in one order, and ONE member also carries long stretches of its own in front of and between its
blocks -- one path lies far away while the others are at hand, the shape that csrc/rv_pick_multi_chain.hip names as reaching its gap bound; the far
member is the first sequence of some jobs and the last of others, so that the high position bits also stand next to the highest sample id; `far-swapped`:
two of the blocks are swapped in a subset of the members (many_chain_wide_cases.shuffled / tied), so that the weights decide the chain.  Sizes: the small
classes have jobs of exactly 2048 ranks, the large classes two jobs of exactly 2^17 ranks each (far member first / last: relative positions with bit 16
set on path 0 and on path 1, in sample 0 and in sample 15) and one of 2^17 + 1, the first size refused.  Neighbours: a few jobs of the class' existing
`rearranged` / `shuffled` / `tied` generators at new seeds.  Deterministic; the sequences are generated, not stored.  The expected results
(tests/golden/many_chain_limits.json, written by tools/gen_many_chain_limits_golden.py) come from `rem.align` on the REFERENCE's own index module."""
import json
import os
import random

import many_cases as mc
import many_chain_cases as cc
import many_chain_large_cases as cp
import many_chain_large_multi_cases as cl
import many_chain_multi_cases as cm
import many_chain_wide_cases as cw
import many_multi_cases as mm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "many_chain_limits.json")

CLASSES = ("chain", "chain_multi", "chain_wide", "chain_large", "chain_large_multi")
LARGE_CLASSES = ("chain_large", "chain_large_multi")
SET_NAMES = ("default", "wmax", "pen-max", "score-max", "score-nopen", "wmax-avg", "wmax-med", "over")
MINLENGTH = dict(chain=20, chain_multi=20, chain_wide=5, chain_large=20, chain_large_multi=20)      # (5: as the weight sets of many_chain_wide_cases)
TOP = 1 << 17            # RV_PICK_CHAIN_RANKS: the last size the large classes admit
BIG = dict(seedsize=200000, maxmums=200000)      # what admits a job of 2^17 ranks (rem.align's defaults of 10 000 would not), as the BIG_SETs of the siblings


def wmax(cls):
    """the class' own weight bound: RV_LEAF_CHAIN_WMAX, RV_LEAF_MCHAIN_WMAX (three classes), RV_PICK_MCHAIN_WMAX"""
    from reveal_amd import many
    return dict(chain=many.CHAIN_WMAX, chain_multi=many.CHAIN_MULTI_WMAX, chain_wide=many.CHAIN_MULTI_WMAX, chain_large=many.CHAIN_MULTI_WMAX,
                chain_large_multi=many.CHAIN_LARGE_MULTI_WMAX)[cls]


def sets(cls, big=False):
    """-> ((name, keyword arguments of rem.align), ..) of a class, (wscore, wpen) as the module says; big: for the jobs of 2^17 and 2^17 + 1 ranks"""
    W = wmax(cls)
    weights = (("default", 1, 1, None), ("wmax", W, W, None), ("pen-max", 1, W, None), ("score-max", W, 1, None), ("score-nopen", W, 0, None),
               ("wmax-avg", W, W, "star-avg"), ("wmax-med", W, W, "star-med"), ("over", W + 1, W + 1, None))
    out = []
    for name, ws, wp, model in weights:
        kw = dict(minlength=MINLENGTH[cls], wscore=ws, wpen=wp)
        if model:
            kw["gcmodel"] = model
        if big:
            kw.update(BIG)
        out.append((name, kw))
    assert tuple(n for n, _ in out) == SET_NAMES
    return tuple(out)


def far(rng, k, total, first, nb, blen, spacer, swapped=False):
    """k members share nb blocks of blen[0] .. blen[1] bases exactly, in one order; k - 1 of them have 0 .. spacer bases of their own between consecutive
    blocks, and the far member -- the first sequence if `first`, else the last -- spends what is left of `total` ranks on stretches of its own: half of
    it in front of its first block, the rest in equal parts between the blocks.  swapped: two blocks are swapped in a random proper subset of the members"""
    blocks = [mc.rnd(rng, n) for n in rng.sample(range(blen[0], blen[1] + 1), nb)]
    order = list(range(nb))
    sub = set()
    if swapped:
        i, j = rng.sample(range(nb), 2); order[i], order[j] = order[j], order[i]
        sub = set(rng.sample(range(k), rng.randint(1, k - 1)))
    at = 0 if first else k - 1
    out = []
    for s in range(k):
        if s == at:
            out.append(None)
            continue
        t = ""
        for q, b in enumerate(order if s in sub else range(nb)):
            if q:
                t += mc.rnd(rng, rng.randint(0, spacer))
            t += blocks[b]
        out.append(t)
    own = total - k - sum(len(t) for t in out if t is not None) - sum(map(len, blocks))
    assert own >= 2 * nb, (k, total, own)
    parts = [own // 2] + [(own - own // 2) // (nb - 1)] * (nb - 1)
    parts[-1] += own - sum(parts)
    out[at] = "".join(mc.rnd(rng, parts[q]) + blocks[b] for q, b in enumerate(order if at in sub else range(nb)))
    assert mm.ranks(out) == total
    return out


# per class: (k, ranks, far member first, blocks, (shortest, longest block), most spacer bases, swapped) of its `far` jobs; the jobs of the large classes
# at 2^17 and 2^17 + 1 ranks come last (BIG_JOBS of them, under sets(cls, big=True))
FAR = dict(
    chain=((2, 2048, True, 4, (40, 90), 6, False), (2, 2048, False, 5, (40, 90), 6, False), (2, 1201, True, 3, (30, 60), 6, False),
           (2, 777, False, 4, (25, 50), 6, False), (2, 2048, False, 5, (40, 90), 6, True), (2, 1500, True, 4, (40, 90), 6, True)),
    chain_multi=((3, 2048, False, 4, (30, 60), 6, False), (16, 2048, True, 3, (21, 27), 3, False), (3, 1333, True, 5, (25, 50), 6, False),
                 (16, 2048, False, 3, (21, 27), 3, False), (5, 2048, False, 4, (25, 40), 6, False), (3, 2048, True, 4, (30, 60), 6, True),
                 (8, 1999, False, 4, (22, 32), 4, True)),
    chain_wide=((17, 2048, False, 3, (7, 12), 2, False), (64, 2048, True, 3, (5, 8), 1, False), (17, 1501, True, 4, (7, 12), 2, False),
                (64, 2048, False, 3, (5, 8), 1, False), (33, 2048, False, 3, (6, 10), 2, False), (17, 2048, True, 4, (7, 12), 2, True),
                (33, 1777, False, 3, (6, 10), 2, True)),
    chain_large=((2, 9000, True, 4, (150, 400), 12, False), (2, 6001, False, 5, (100, 300), 12, False), (2, 3003, True, 3, (60, 200), 12, False),
                 (2, 2100, False, 4, (40, 120), 12, False), (2, 8191, False, 5, (150, 400), 12, True), (2, 4500, True, 4, (100, 300), 12, True),
                 (2, TOP, True, 5, (200, 600), 12, False), (2, TOP, False, 4, (200, 600), 12, False), (2, TOP + 1, True, 4, (200, 600), 12, False)),
    chain_large_multi=((3, 6000, True, 4, (100, 250), 12, False), (16, 9000, False, 4, (40, 90), 8, False), (5, 4001, False, 3, (60, 150), 12, False),
                       (8, 2100, True, 3, (30, 50), 6, False), (3, 7777, False, 5, (100, 250), 12, True), (16, 5000, True, 4, (30, 60), 8, True),
                       (16, TOP, True, 4, (150, 350), 12, False), (16, TOP, False, 5, (150, 350), 12, False), (16, TOP + 1, False, 4, (150, 350), 12, False)),
)
BIG_JOBS = 3             # of a large class: 2^17 ranks with the far member first, with it last, and 2^17 + 1 ranks
N_NEIGHBOURS = dict(chain=6, chain_multi=5, chain_wide=4, chain_large=5, chain_large_multi=4)
# (far jobs, neighbours).  chain's neighbours: the first seed from 202 on at which the reference's results under pen-max differ from default's on three of
# the six jobs -- fixture condition (b); its far jobs cannot help there: with ONE path the longer side of every gap, a pair's gap costs | |d0| - |d1| |
# add up to one sum whatever the chain takes, and what a chain leaves out the recursion finds in a child
SEEDS = dict(chain=(201, 204), chain_multi=(203, 204), chain_wide=(205, 206), chain_large=(207, 208), chain_large_multi=(209, 210))


def neighbours(cls):
    """jobs of the class' existing generators at a seed of this module's -> [(class name, [seq, ..])]"""
    rng = random.Random(SEEDS[cls][1])
    n = N_NEIGHBOURS[cls]
    if cls == "chain":
        return [("rearranged", list(cc.rearranged(rng))) for _ in range(n)]
    if cls == "chain_multi":
        def fit(fam):
            return [s[:(mm.MAX_RANKS - len(fam)) // len(fam)] for s in fam] if mm.ranks(fam) > mm.MAX_RANKS else list(fam)
        return [("rearranged", fit(cm.rearranged(rng, mm.K_VALUES[j % len(mm.K_VALUES)]))) for j in range(n)]
    if cls == "chain_wide":
        return [("tied" if j % 2 else "shuffled", (cw.tied if j % 2 else cw.shuffled)(rng, (17, 33, 64, 48)[j % 4])) for j in range(n)]
    if cls == "chain_large":
        return [("rearranged-large", list(cp.rearranged_large(rng))) for _ in range(n)]
    return [("tied" if j % 2 else "shuffled", cl.blocks_family(rng, cl.K_VALUES[(2 * j + 1) % len(cl.K_VALUES)], bool(j % 2))) for j in range(n)]


_JOBS = {}


def jobs(cls):
    """-> [(class name, [seq, ..])] of a class: its `far` / `far-swapped` jobs below 2^17 ranks, its neighbours, and for a large class its BIG_JOBS jobs
    of 2^17, 2^17 and 2^17 + 1 ranks last (built once per process: nobody changes the list)"""
    if cls not in _JOBS:
        rng = random.Random(SEEDS[cls][0])
        made = [("far-swapped" if spec[6] else "far", far(rng, *spec)) for spec in FAR[cls]]
        nbig = BIG_JOBS if cls in LARGE_CLASSES else 0
        small = made[:len(made) - nbig]
        _JOBS[cls] = small + neighbours(cls) + made[len(made) - nbig:]
    return [(c, list(f)) for c, f in _JOBS[cls]]


def is_big(cls, j):
    """whether job j of the class runs under sets(cls, big=True): the last BIG_JOBS jobs of a large class"""
    return cls in LARGE_CLASSES and j >= len(FAR[cls]) - BIG_JOBS + N_NEIGHBOURS[cls]


def fillers(cls):
    """small jobs that bring the call with the jobs of 2^17 ranks up to the class' threshold of admitted jobs (RV_MANY_CHAIN_LARGE_MIN = 4 /
    RV_MANY_CHAIN_LARGE_MULTI_MIN = 4; the two big jobs count): the class' first two `far` jobs.  They run under that call's seedsize and maxmums
    (BIG), which change nothing for them -- the generator checks it --, so the golden results of the plain sets hold for them there"""
    return [f for _, f in jobs(cls)[:2]]


def switch(cls):
    """the keyword of align_many / takes_shared_launch that turns the class on"""
    return {cls: True}


picker_args = cc.picker_args
run_kw = cm.run_kw
rem_align_job = cc.rem_align_job
sha = cc.sha


def begins_of(seqs):
    """where every sequence begins in the job's text `s0$s1$..`"""
    out, at = [], 0
    for s in seqs:
        out.append(at)
        at += len(s) + 1
    return out


def relative_positions(seqs, anchors):
    """-> per sequence index the largest position of any anchor member relative to its sequence's begin (-1: no anchor has a member there)"""
    beg = begins_of(seqs)
    top = [-1] * len(seqs)
    for _, pos in anchors:
        for p in pos:
            q = max(s for s in range(len(beg)) if beg[s] <= p)
            top[q] = max(top[q], p - beg[q])
    return top


def rem_align_recorded(seqs, ext, indexmod=None, **kw):
    """cc.rem_align_job that also watches schemes.chain -> (sorted anchors, final text); ext: dict(score=, penalty=) raised to the largest |score| of
    any member of a returned chain and the largest wpen x gapcost between consecutive members of one (the left sentinel in front of the first)"""
    from reveal_amd import schemes
    orig = schemes.chain

    def watch(mums, left, right, gcmodel="sumofpairs", wscore=1, wpen=1):
        r = orig(mums, left, right, gcmodel=gcmodel, wscore=wscore, wpen=wpen)
        keys = sorted(left[2])
        end = [left[2][q] for q in keys]          # (the sentinel is a match of length 0)
        for mum, sc in r:
            ext["score"] = max(ext["score"], abs(int(sc)))
            ext["penalty"] = max(ext["penalty"], int(wpen) * schemes.gapcost(end, [mum[2][q] for q in keys], gcmodel))
            end = [mum[2][q] + mum[0] for q in keys]
        return r
    schemes.chain = watch
    try:
        return cc.rem_align_job(seqs, indexmod=indexmod, **kw)
    finally:
        schemes.chain = orig


def load_golden():
    """-> ({class: {set name: [(sorted anchors [(l, (members in emitted order))], sha256 of the final text)] in the order of jobs(class)}},
    {class: dict(score={set: largest |score|}, penalty={set: largest wpen x gapcost}, positions=[per job [per sequence index the largest relative
    position of an anchor, over every set]])}).  The file keeps a result an earlier set already has only once ("same")."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["sets"] == list(SET_NAMES) and doc["classes"] == list(CLASSES)
    out = {}
    for cls in CLASSES:
        assert doc["jobs"][cls] == len(jobs(cls))
        res = out[cls] = {}
        for n in SET_NAMES:
            res[n] = [res[r["same"]][j] if "same" in r else ([(a[0], tuple(a[1:])) for a in r["anchors"]], r["sha"]) for j, r in enumerate(doc["results"][cls][n])]
    return out, doc["extremes"]
