"""inputs of the align_many tests with the reference's default picker on jobs of 17 .. 64 sequences (RV_MANY_CHAIN_WIDE;
tests/test_cpu_many_chain_wide.py checks the list and the golden file, tests/test_gpu_many_chain_wide.py runs it): the class jobs and the short
jobs of many_wide_cases, the corner jobs the wide small rounds take, and two classes of its own whose chains have something to decide -- on
the families of many_wide_cases alone the reference returns the same anchors whatever the weights and the gap model are, and the gap costs over up
to 64 paths would go untested.  "shuffled": blocks of distinct lengths, two of them swapped in a subset of the members -- the weights and sum of pairs
decide there.  The star models do not: `|sum d| / k` is what a chain leaves uncovered, and the median follows it, so with blocks of distinct lengths
they choose what the gains choose, and star-avg and star-med return what wpen=0 returns.  "tied": the two swapped blocks have EQUAL lengths, the gains
tie, and the gap cost alone decides -- star-avg by its truncation per gap, star-med by where the majority's spacers lie.  Deterministic.  The expected results (tests/golden/many_chain_wide.json, written by
tools/gen_many_chain_wide_golden.py) come from `rem.align` on the REFERENCE's own index module."""
import hashlib
import json
import os
import random

import many_cases as mc
import many_chain_cases as cc
import many_chain_multi_cases as cm
import many_multi_cases as mm
import many_wide_cases as mw

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "many_chain_wide.json")

# (name, keyword arguments of rem.align); what is not named: wpen 1, wscore 1, sumofpairs, trim, seedsize 10000, maxmums 10000, minn 2
SETS = (
    ("default", dict(minlength=20)),
    ("minl10", dict(minlength=10)),
    ("minl5", dict(minlength=5)),
    ("minl1", dict(minlength=1)),
    ("minn3", dict(minlength=10, minn=3)),
    ("minn17", dict(minlength=10, minn=17)),
    ("wpen4", dict(minlength=5, wpen=4)),
    ("wpen0", dict(minlength=5, wpen=0)),
    ("wscore3", dict(minlength=5, wscore=3)),
    ("star-avg", dict(minlength=5, gcmodel="star-avg")),
    ("star-med", dict(minlength=5, gcmodel="star-med")),
)
WEIGHT_SETS = ("wpen4", "wpen0", "wscore3", "star-avg", "star-med")      # each compared with minl5: fixture condition (d)
HASHED_SETS = ("minl1",)      # the file keeps the anchor count and a SHA-256 of the anchor list for these sets, the anchors themselves for the others
PER_K = 8                         # many_wide_cases.class_jobs(PER_K): every class once per k
SHORT_PER_K = 6
N_SHUFFLED = 40
SHUFFLED_K = (17, 24, 32, 48, 64)
CORNERS = ("k17_single_bases", "k64_single_bases", "k17", "k64_full")
N_TIED = 24
TIED_K = (17, 33, 48, 64)


def shuffled(rng, k):
    """k members share 3 .. 5 blocks of distinct lengths exactly; two of the blocks are swapped in a random proper subset of the members; between
    consecutive blocks every member has a spacer of 0 .. g bases of its own.  Blocks sized so the job stays within 2048 ranks (7 bases at k = 64)"""
    L = (mw.MAX_RANKS - k) // k
    nb = 3 if L < 40 else rng.randint(3, 5)
    g = max(2, min(12, (L // nb) // 3))
    bl = (L - (nb - 1) * g) // nb
    lo = max(5, bl - 6)
    lens = rng.sample(range(lo, bl + 1), min(nb, bl + 1 - lo))
    while len(lens) < nb:
        lens.append(rng.randint(lo, bl))
    blocks = [mc.rnd(rng, n) for n in lens]
    order = list(range(nb)); i, j = rng.sample(range(nb), 2); order[i], order[j] = order[j], order[i]
    sub = set(rng.sample(range(k), rng.randint(1, k - 1)))
    out = []
    for s in range(k):
        t = ""
        for q, b in enumerate(order if s in sub else range(nb)):
            if q:
                t += mc.rnd(rng, rng.randint(0, g))
            t += blocks[b]
        out.append(t)
    assert mm.ranks(out) <= mw.MAX_RANKS
    return out


def tied(rng, k):
    """`shuffled` with the two swapped blocks of EQUAL length (the other blocks one to three bases shorter): the chain has to choose between two
    matches of one gain, and the gap cost decides"""
    L = (mw.MAX_RANKS - k) // k
    nb = 3 if L < 40 else rng.randint(3, 4)
    g = max(2, min(12, (L // nb) // 3))
    bl = (L - (nb - 1) * g) // nb
    i, j = rng.sample(range(nb), 2)
    lens = [bl if q in (i, j) else max(5, bl - rng.randint(1, 3)) for q in range(nb)]
    blocks = [mc.rnd(rng, n) for n in lens]
    order = list(range(nb)); order[i], order[j] = order[j], order[i]
    sub = set(rng.sample(range(k), rng.randint(1, k - 1)))
    out = []
    for s in range(k):
        t = ""
        for q, b in enumerate(order if s in sub else range(nb)):
            if q:
                t += mc.rnd(rng, rng.randint(0, g))
            t += blocks[b]
        out.append(t)
    assert mm.ranks(out) <= mw.MAX_RANKS
    return out


def flagged_job():
    """the sixth `shuffled` job at seed 93 (17 sequences): at minlength 1 one of its sub-indices holds two matches with the split's offsets member by
    member, where the kernel gives up (flag 8) and the job finishes on the ordinary path -- the one job found so far that the kernel flags by itself"""
    rng = random.Random(93)
    return [shuffled(rng, SHUFFLED_K[j % len(SHUFFLED_K)]) for j in range(6)][5]


def jobs():
    """-> [(class, [seq, ..])]: many_wide_cases.class_jobs(PER_K), short_jobs(SHORT_PER_K), the corner jobs the wide small rounds take, N_SHUFFLED
    `shuffled` jobs (k cycling 17, 24, 32, 48, 64), N_TIED `tied` jobs (k cycling 17, 33, 48, 64)"""
    out = [(cls, list(fam)) for cls, k, fam in mw.class_jobs(PER_K)]
    out += [("short", list(fam)) for fam in mw.short_jobs(SHORT_PER_K)]
    corners = {name: fam for name, fam, _ in mw.corner_jobs()}
    out += [("corner:" + name, list(corners[name])) for name in CORNERS]
    # (the seed: the first from 93 on at which tools/chain_multi_proto.py --cases wide reports no give-up of the kernel's pick stage under any set -- at 93
    # one job at minlength 1 holds two matches with the split's offsets, the kernel would flag it, and the GPU tests could not ask for every job shared)
    rng = random.Random(94)
    out += [("shuffled", shuffled(rng, SHUFFLED_K[j % len(SHUFFLED_K)])) for j in range(N_SHUFFLED)]
    # (the seed: the first at which the prototype reports no give-up under any set, as above, AND the reference's star-avg and star-med results differ
    # on five jobs or more -- fixture condition (f); at seeds 1 and 2 a job gives up at minlength 1, or the two models differ on 2 jobs only)
    rng = random.Random(3)
    return out + [("tied", tied(rng, TIED_K[j % len(TIED_K)])) for j in range(N_TIED)]


picker_args = cc.picker_args
run_kw = cm.run_kw
rem_align_job = cc.rem_align_job
sha = cc.sha
sample_sets = cm.sample_sets
kernel_scan = cm.kernel_scan


def anchors_sha(anchors):
    """SHA-256 of the canonical anchor list: sorted [(l, (members in emitted order))] as compact JSON"""
    return hashlib.sha256(json.dumps([[int(l)] + [int(p) for p in pos] for l, pos in anchors], separators=(",", ":")).encode()).hexdigest()


def record(name, anchors, text):
    """a result as the file keeps it"""
    if name in HASHED_SETS:
        return dict(n=len(anchors), asha=anchors_sha(anchors), sha=sha(text))
    return dict(anchors=[[l] + list(p) for l, p in anchors], sha=sha(text))


def same(rec, anchors, text_sha):
    """whether a result (sorted anchors, sha256 of the final text) is the one the file keeps"""
    if "anchors" in rec:
        return [[l] + list(p) for l, p in anchors] == rec["anchors"] and text_sha == rec["sha"]
    return len(anchors) == rec["n"] and anchors_sha(anchors) == rec["asha"] and text_sha == rec["sha"]


def resolve(results):
    """the results of the file with its references (dict(same_as=set name): the job's result equals that set's) followed"""
    def follow(r, j):
        while "same_as" in r:
            r = results[r["same_as"]][j]
        return r
    return {n: [follow(r, j) for j, r in enumerate(rs)] for n, rs in results.items()}


def load_golden():
    """-> {set name: [record in the order of jobs()]}: dict(anchors=[[l, member, ..]], sha=of the final text), or dict(n, asha, sha) for HASHED_SETS;
    compare with same()"""
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["sets"] == [n for n, _ in SETS] and doc["jobs"] == len(jobs())
    res = resolve(doc["results"])
    return {n: res[n] for n, _ in SETS}
