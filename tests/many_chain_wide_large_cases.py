"""inputs of the align_many tests with the reference's default picker for jobs of 17 .. 64 sequences above 2048 ranks (RV_MANY_CHAIN_WIDE_LARGE;
tests/test_cpu_many_chain_wide_large.py checks the list and the golden file, tests/test_gpu_many_chain_wide_large.py runs it): the `shuffled`, `tied`
and `subset` families of many_chain_large_multi_cases scaled to k in (17, 32, 33, 48, 64) -- 33 is the first k that uses the high word of a 64-bit
sample set -- at 2100 .. 6000 ranks, a few of many_wide_cases' large jobs, and the corners: 17 sequences at 2049 ranks, 64 sequences of 32 bases (2112
ranks), a one-base sequence, and one job whose positions need 17 bits.  Deterministic.  The expected results
(tests/golden/many_chain_wide_large.json, written by tools/gen_many_chain_wide_large_golden.py) come from `rem.align` on the REFERENCE's own index
module.

What the `subset` family is here: k - 1 members SUBSET_DIVERGENCE apart and one that shares nothing with them.  Where no match lies in every sample the
picker chains the whole list, and k_pick_multi_chain<64> holds at most 256 candidates of a sub-index (fixture condition (g)); see SUBSET_DIVERGENCE."""
import os
import random

import many_cases as mc
import many_chain_large_multi_cases as cl
import many_multi_cases as mm
import many_wide_cases as mw

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "many_chain_wide_large.json")

SETS = cl.SETS                                       # weights 0 .. 4: inside the class' bound of 128
WEIGHT_SETS = cl.WEIGHT_SETS                         # each compared with default: fixture condition (f)
# the job whose positions need 17 bits runs under a set of its own: rem.align's default seedsize and maxmums would not admit it
BIG_SET = ("big", dict(minlength=20, seedsize=200000, maxmums=200000))
K_VALUES = (17, 32, 33, 48, 64)
CAP = 256                                            # RV_PICK_WCHAIN_CAP_MAX: the candidates k_pick_multi_chain<64> holds per sub-index
N_SHUFFLED = 10
N_TIED = 10
N_SUBSET = 5
N_WIDE = 3                                           # many_wide_cases.large_jobs(N_WIDE): sites, identical, dropout at k = 17, 33, 64
RANKS = (2100, 6000)
BIG_FROM = 66000                                     # where the last piece of the big job lies in its first sequence
# many_chain_large_multi_cases.subset_family has its members 1 % apart.  At these k that breaks fixture condition (g): the reference's picker sees 403
# candidates at the root of the job of 33 sequences and 389 / 308 at and below the root of the job of 64.  The DIVERGENCE is shrunk, to 0.5 %, until the
# reference alone stays inside the cap of 256; the sequences keep their lengths (the generator prints the counts, the fixture's `roots` / `below` keep them).
SUBSET_DIVERGENCE = 0.005


def blocks_family(rng, k, equal):
    """many_chain_large_multi_cases.blocks_family at these k: k members share three blocks exactly (4 .. 6 from 400 bases a member on), two of the blocks are swapped in a random proper
    subset of the members, between consecutive blocks every member has a spacer of 0 .. g bases of its own; equal: the two swapped blocks have ONE
    length (the others are one or two bases shorter).  Members of at least 87 bases, so that three blocks of 22 bases and more fit: every block is a
    match at minlength 20"""
    total = rng.randint(max(RANKS[0] + 300, 88 * k + k), RANKS[1] - 100)
    L = (total - k) // k
    nb = rng.randint(4, 6) if L >= 400 else 3
    g = max(2, min(12, (L // nb) // 4))
    bl = (L - (nb - 1) * g) // nb
    lo = max(20, bl - 12)
    assert bl - lo + 1 >= nb and bl >= 22, (k, L, bl)
    i, j = rng.sample(range(nb), 2)
    if equal:
        lens = [bl if q in (i, j) else bl - rng.randint(1, 2) for q in range(nb)]
    else:
        lens = rng.sample(range(lo, bl + 1), nb)
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
    """k - 1 members SUBSET_DIVERGENCE apart and one that shares nothing with them: no match lies in every sample"""
    total = rng.randint(max(RANKS[0] + 100, 60 * k), RANKS[1] - 100)
    L = (total - k) // k
    base = mc.rnd(rng, L)
    fam = [mc.mutate(rng, base, SUBSET_DIVERGENCE) for _ in range(k)]
    fam[rng.randrange(k)] = mc.rnd(rng, L)
    assert RANKS[0] <= mm.ranks(fam) <= RANKS[1]
    return fam


def corner_jobs():
    """-> [(class, [seq, ..])]: 17 sequences at 2049 ranks, the first count above 2048; 64 sequences of 32 bases, 2112 ranks; a one-base sequence among
    20 (2871 ranks)"""
    rng = random.Random(111)
    first = mw.with_sites(rng, mc.rnd(rng, 120), 17)
    first[16] = first[16][:112]
    k64 = mw.with_sites(rng, mc.rnd(rng, 32), 64)
    one = mw.with_sites(rng, mc.rnd(rng, 150), 20)
    one[rng.randrange(20)] = rng.choice("ACGT")
    assert [mm.ranks(f) for f in (first, k64, one)] == [2049, 2112, 2871]
    return [("corner:k17_2049", first), ("corner:k64_2112", k64), ("corner:one_base", one)]


def big_job():
    """a sequence of 70 000 bases and 16 pieces of it (from 3000, 7200, .. 66 000 on): fifteen of 3000 bases with about one base in a thousand
    substituted, the last of 3500 bases with two substitutions.  118 517 ranks in 17 sequences.  The pieces do not overlap, so no match lies in every
    sample, the root holds every pair match -- a few per piece: inside the cap -- and `segment` chooses the last piece's (the largest sum of lengths):
    the chain, the split and the children work at positions of the first sequence from BIG_FROM = 66 000 on, which need 17 bits"""
    rng = random.Random(114)
    base = mc.rnd(rng, 70000)
    fam = [base] + [mc.mutate(rng, base[3000 + 4200 * i:6000 + 4200 * i], 0.001) for i in range(15)]
    last = list(base[BIG_FROM:BIG_FROM + 3500])
    for p in (1000, 2200):
        last[p] = "ACGT"[("ACGT".index(last[p].upper()) + 1) % 4]
    fam.append("".join(last))
    assert len(fam) == 17 and mm.ranks(fam) == 118517 <= 1 << 17 and BIG_FROM > 1 << 16
    return fam


def fillers(count):
    """small jobs of the class that bring the call with the big job up to RV_MANY_CHAIN_WIDE_LARGE_MIN admitted jobs"""
    rng = random.Random(115)
    return [mw.with_sites(rng, mc.rnd(rng, 125), 17) for _ in range(count)]      # 17 x 126 = 2142 ranks


def jobs():
    """-> [(class, [seq, ..])]: N_SHUFFLED `shuffled`, N_TIED `tied` and N_SUBSET `subset` jobs (k cycling 17, 32, 33, 48, 64), many_wide_cases'
    large jobs (sites, identical, dropout at k = 17, 33, 64), the three corners"""
    rng = random.Random(111)
    out = [("shuffled", blocks_family(rng, K_VALUES[j % len(K_VALUES)], False)) for j in range(N_SHUFFLED)]
    rng = random.Random(112)
    out += [("tied", blocks_family(rng, K_VALUES[j % len(K_VALUES)], True)) for j in range(N_TIED)]
    rng = random.Random(113)
    out += [("subset", subset_family(rng, K_VALUES[j % len(K_VALUES)])) for j in range(N_SUBSET)]
    out += [("wide:" + cls, list(fam)) for cls, k, fam in mw.large_jobs(N_WIDE)]
    return out + corner_jobs()


picker_args = cl.picker_args
run_kw = cl.run_kw
rem_align_job = cl.rem_align_job
rem_align_recorded = cl.rem_align_recorded
sha = cl.sha
digest = cl.digest


def load_golden():
    """-> {set name: [(sorted anchors [(l, (members in emitted order))], sha256 of the final text)] in the order of jobs()}, "big": the one entry of the
    big job, "roots": per job under `default` (candidates at the root, samples, members of the first pick, whether `segment` chose the set), "below":
    the most candidates of any sub-index below the root, "big_most": the most candidates of any sub-index of the big job.  The file keeps a result an
    earlier set already has only once ("same")."""
    import json
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
    out["big_most"] = doc["big_most"]
    return out
