"""inputs of the align_many tests with the reference's default picker for jobs of 3 .. 16 sequences above 2048 ranks (RV_MANY_CHAIN_LARGE_MULTI;
tests/test_cpu_many_chain_large_multi.py checks the list and the golden file, tests/test_gpu_many_chain_large_multi.py runs it): the class jobs of
many_large_multi_cases, the `shuffled` and `tied` families of many_chain_wide_cases scaled to 2100 .. 6000 ranks -- where trimming and chaining choose
other anchors than the longest match --, a `subset` class in which one member shares nothing with the others, so that no match lies in every sample,
`segment` chooses a sample subset at the root and a `rest` child exists, and the corners: 2049 ranks with three sequences, sixteen sequences at 2064
ranks, a one-base sequence, and one job whose positions need 17 bits.  Deterministic.  The expected results (tests/golden/many_chain_large_multi.json,
written by tools/gen_many_chain_large_multi_golden.py) come from `rem.align` on the REFERENCE's own index module."""
import hashlib
import json
import os
import random

import many_cases as mc
import many_chain_cases as cc
import many_chain_multi_cases as cm
import many_large_multi_cases as lm
import many_multi_cases as mm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "many_chain_large_multi.json")

# (name, keyword arguments of rem.align); what is not named: wpen 1, wscore 1, sumofpairs, trim, seedsize 10000, maxmums 10000, minn 2
# (many_chain_cases.SETS without minl1 -- star-avg and star-med are among them -- and wpen0, which fixture condition (c) asks for)
SETS = tuple((n, kw) for n, kw in cc.SETS if n != "minl1") + (("wpen0", dict(minlength=20, wpen=0)),)
WEIGHT_SETS = ("wpen0", "star-avg", "star-med")      # each compared with default: fixture condition (c)
# the job whose positions need 17 bits runs under a set of its own: rem.align's default seedsize and maxmums would not admit it
BIG_SET = ("big", dict(minlength=20, seedsize=200000, maxmums=200000))
K_VALUES = lm.K_VALUES                               # (3, 4, 5, 8, 16)
PER_CLASS = 2
N_SHUFFLED = 10
N_TIED = 10
N_SUBSET = 6
RANKS = (2100, 6000)


def blocks_family(rng, k, equal):
    """many_chain_wide_cases.shuffled / tied at these sizes: k members share 4 .. 6 blocks exactly, two of the blocks are swapped in a random proper
    subset of the members, between consecutive blocks every member has a spacer of 0 .. 12 bases of its own; equal: the two swapped blocks have ONE
    length (the others are one to three bases shorter), so the chain has to choose between two matches of one gain and the gap cost decides"""
    total = rng.randint(max(RANKS[0] + 300, 220 * k), RANKS[1] - 100)
    L = (total - k) // k
    nb = rng.randint(4, 6) if L >= 400 else 3
    g = 12
    bl = (L - (nb - 1) * g) // nb
    i, j = rng.sample(range(nb), 2)
    if equal:
        lens = [bl if q in (i, j) else bl - rng.randint(1, 3) for q in range(nb)]
    else:
        lens = rng.sample(range(bl - 12, bl + 1), nb)
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
    assert RANKS[0] <= mm.ranks(out) <= RANKS[1]
    return out


def subset_family(rng, k):
    """k - 1 members 1 % apart and one that shares nothing with them: no match lies in every sample"""
    total = rng.randint(RANKS[0] + 100, RANKS[1] - 100)
    L = (total - k) // k
    base = mc.rnd(rng, L)
    fam = [mc.mutate(rng, base, 0.01) for _ in range(k)]
    fam[rng.randrange(k)] = mc.rnd(rng, L)
    return fam


def corner_jobs():
    """-> [(class, [seq, ..])]: 2049 ranks with k = 3; k = 16 at 2064 ranks; a one-base sequence (many_large_multi_cases.corner_jobs' own)"""
    c = lm.corner_jobs()
    assert [mm.ranks(c[j]) for j in (0, 2, 3)] == [2049, 2064, 3004]
    return [("corner:ranks_2049", list(c[0])), ("corner:k16_2064", list(c[2])), ("corner:one_base", list(c[3]))]


def big_job():
    """a sequence of 70 000 bases and two pieces of it of 30 000 (from 40 000 and from 35 000 on), 1 % apart: 130 003 ranks, the matches of the first
    sequence lie at positions that need 17 bits"""
    rng = random.Random(104)
    base = mc.rnd(rng, 70000)
    fam = [mc.mutate(rng, base, 0.01), mc.mutate(rng, base[40000:], 0.01), mc.mutate(rng, base[35000:65000], 0.01)]
    assert mm.ranks(fam) == 130003 and len(fam[0]) > 1 << 16
    return fam


def fillers(count):
    """small jobs that bring the call with the big job up to RV_MANY_CHAIN_LARGE_MULTI_MIN admitted jobs"""
    return [list(f) for f in lm.sized_jobs(count)]


def jobs():
    """-> [(class, [seq, ..])]: many_large_multi_cases.class_jobs(PER_CLASS), N_SHUFFLED `shuffled` and N_TIED `tied` jobs, N_SUBSET `subset` jobs
    (k cycling 3, 4, 5, 8, 16; the subset jobs from 4 on), the three corners"""
    out = [(cls, list(fam)) for cls, k, fam in lm.class_jobs(PER_CLASS)]
    rng = random.Random(101)
    out += [("shuffled", blocks_family(rng, K_VALUES[j % len(K_VALUES)], False)) for j in range(N_SHUFFLED)]
    rng = random.Random(102)
    out += [("tied", blocks_family(rng, K_VALUES[j % len(K_VALUES)], True)) for j in range(N_TIED)]
    rng = random.Random(103)
    out += [("subset", subset_family(rng, K_VALUES[1 + j % (len(K_VALUES) - 1)])) for j in range(N_SUBSET)]
    return out + corner_jobs()


picker_args = cc.picker_args
run_kw = cm.run_kw
rem_align_job = cc.rem_align_job
sha = cc.sha


def rem_align_recorded(seqs, indexmod=None, **kw):
    """cc.rem_align_job that also watches the picker -> (sorted anchors [(l, (members in the order graphalign got them))], final text, calls): calls =
    one (candidates, samples of the sub-index, members of the pick or 0, whether `segment` chose the set) per picker call with a non-empty match list,
    the root's first.  candidates: what the picker chains -- the matches in every sample of the sub-index, or, where there is none, all of the list
    (csrc/rv_pick_multi_chain.hip counts the same against its cap)"""
    from reveal_amd import schemes
    calls = []
    orig = schemes.GraphPicker.graphmumpicker

    def watch(self, mums, idx, precomputed=False, minlength=0):
        r = orig(self, mums, idx, precomputed, minlength)
        if len(mums):
            ns = idx.nsamples
            full = sum(1 for m in mums if m[1] == ns)
            calls.append((full if full else len(mums), ns, int(r[0][1]) if r else 0, full == 0 and ns > 2))
        return r
    schemes.GraphPicker.graphmumpicker = watch
    try:
        an, T = cc.rem_align_job(seqs, indexmod=indexmod, **kw)
    finally:
        schemes.GraphPicker.graphmumpicker = orig
    return an, T, calls


def digest(anchors):
    return hashlib.sha256(json.dumps([[l] + list(p) for l, p in anchors], separators=(",", ":")).encode()).hexdigest()


def load_golden():
    """-> {set name: [(sorted anchors [(l, (members in emitted order))], sha256 of the final text)] in the order of jobs()}, "big": the one entry of the
    big job, "roots": per job under `default` (candidates at the root, samples, members of the first pick, whether `segment` chose), "below": the most
    candidates of any sub-index below the root.  The file keeps a result an earlier set already has only once ("same")."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["sets"] == [n for n, _ in SETS] and doc["jobs"] == len(jobs())
    out = {}

    def entry(r):
        return ([(a[0], tuple(a[1:])) for a in r["anchors"]], r["sha"])
    for n, _ in SETS:
        out[n] = [out[r["same"]][j] if "same" in r else entry(r) for j, r in enumerate(doc["results"][n])]
    out["big"] = [entry(doc["big"])]
    out["roots"] = [tuple(r) for r in doc["roots"]]
    out["below"] = doc["below"]
    return out
