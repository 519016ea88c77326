"""inputs of the mums_many tests for jobs above 2048 ranks (RV_MANY_SCAN_LARGE; tests/test_cpu_many_mums_large.py checks them,
tests/test_gpu_many_mums_large.py uses them): the smallest shapes at which the segmented build on the round's text in place, and the scan kernels over
segments of more than 2048 ranks, can go wrong.  A large job has 2049 ranks by definition, so nothing is bigger than a few thousand ranks except the two
jobs at the bound RV_MANY_LARGE_MAX.  The checker is many_mums_cases' (the CPU oracle on the job ALONE).  Sequences are str and are scanned as given
(toupper=False).  Deterministic."""
import functools
import random

import many_cases as mc
import many_multi_cases as mm
import many_mums_cases as C

LEAF_RANKS = 2048         # ranks of the largest job of the small rounds
LARGE_MAX = 1 << 17       # default of RV_MANY_LARGE_MAX: ranks of the largest job of the large rounds

# many_mums_cases.NESTED_LAST behind paddings without T, so that the job has more than 2048 ranks and the only suffixes that begin with T are still
# TA$ < TGA$ < TGCA$ < TGCCA$, one per sample, at the job's last four ranks: the thread of the job's last rank emits (3, n=2), (2, n=3) and (1, n=4).
# The paddings end in different characters, so every interval has a left-maximal adjacent pair -- test_cpu_many_mums_large checks it on the oracle
NESTED_PAD = 520


def nested_last_large(rng):
    ends = "GACG"
    return [mc.rnd(rng, NESTED_PAD - 1, "ACG") + ends[q] + s for q, s in enumerate(C.NESTED_LAST)]


@functools.lru_cache(maxsize=None)
def large_cases(seed=41):
    """-> ((name, (seq, ..), taken by the shared launches with RV_MANY_SCAN_LARGE on), ..)"""
    rng = random.Random(seed)
    x = mc.rnd(rng, 25)
    out = []
    # sizes: both sides of nothing here (2048 | 2049 is many_mums_cases'), the first sizes of the class and the k at which the scan changes its ways
    for n in (2049, 2050, 3000):
        out.append(("pair_ranks_%d" % n, mm.sized_job(rng, 2, n), True))
        out.append(("three_ranks_%d" % n, mm.sized_job(rng, 3, n), True))
    for k, n in ((16, 2049), (17, 2500), (33, 3333), (64, 4000)):
        out.append(("k%d_ranks_%d" % (k, n), mm.sized_job(rng, k, n, 0.02), True))
    # depth of the doubling: h = 5, 10, .. has to pass the longest repeat
    a = mc.rnd(rng, 1100)
    out.append(("identical_pair_1100", [a, a], True))
    unit, left, right = mc.rnd(rng, 5), mc.rnd(rng, 30), mc.rnd(rng, 30)
    out.append(("tandem_family", [left + unit * c + right for c in (112, 110, 113, 112)], True))
    out.append(("identical_five", [mc.rnd(rng, 450)] * 5, True))
    # segment edges
    out.append(("match_at_position_0", [x + "A" + mc.rnd(rng, 1100, "AC"), x + "G" + mc.rnd(rng, 1100, "GT")], True))
    out.append(("nested_last_rank", nested_last_large(rng), True))
    # both sequences end in the same 30 bases: a match that ends at the job's last '$'.  The largest of the cases of a few thousand ranks, so the rounds sorted by
    # size place it last: the 8-byte reads of its last positions meet the padding behind the round's text
    tail = mc.rnd(rng, 30)
    out.append(("match_at_the_end", [mc.rnd(rng, 2000, "AC") + "G" + tail, mc.rnd(rng, 2300, "GT") + "A" + tail], True))
    # side bit and la
    out.append(("first_of_one_base", ["A", mc.rnd(rng, 2100)], True))
    out.append(("second_of_one_base", [mc.rnd(rng, 2100), "A"], True))
    long_one = mc.rnd(rng, 2000)
    out.append(("k64_one_long", [rng.choice("ACGT") for _ in range(40)] + [long_one] + [rng.choice("ACGT") for _ in range(23)], True))
    # characters
    out.append(("maximal_through_N", ["CCA" + "N" + x + "A" + mc.rnd(rng, 1100, "AC"), "GGT" + "N" + x + "T" + mc.rnd(rng, 1100, "GT")], True))
    out.append(("maximal_through_lower", ["CCA" + "g" + x + "A" + mc.rnd(rng, 1100, "AC"), "GTT" + "g" + x + "T" + mc.rnd(rng, 1100, "GT")], True))
    l, r = mc.rnd(rng, 600), mc.rnd(rng, 600)
    out.append(("long_N_run", [l + "N" * 12 + r, mc.mutate(rng, l, 0.01) + "N" * 12 + mc.mutate(rng, r, 0.01)], True))
    out.append(("lower_case", [s.lower() for s in mm.sized_job(rng, 3, 2400)], True))
    # bounds
    out.append(("pair_ranks_large_max", mm.sized_job(rng, 2, LARGE_MAX), True))
    out.append(("pair_ranks_large_max_plus_1", mm.sized_job(rng, 2, LARGE_MAX + 1), False))
    # controls that must not move: small jobs stay in the small rounds, k > 64 and a NUL byte stay ordinary
    for j, p in enumerate(C.pair_batch()[:3]):
        out.append(("small_pair_%d" % j, p, True))
    for j, f in enumerate(C.multi_batch()[:2]):
        out.append(("small_family_%d" % j, f, True))
    out.append(("small_pair_ranks_2048", mm.sized_job(rng, 2, 2048), True))
    out.append(("k65", mm.sized_job(rng, 65, 65 * 40, 0.02), False))
    nul = mc.rnd(rng, 1100)
    out.append(("nul_byte", [nul, nul[:500] + "\0" + nul[501:]], False))
    return tuple((name, tuple(seqs), shared) for name, seqs, shared in out)


def is_large(seqs):
    return C.ranks(seqs) > LEAF_RANKS


def jobs(names=None, without=()):
    """the sequences of the cases (all, or the named ones), as lists"""
    return [list(s) for n, s, _ in large_cases() if (names is None or n in names) and n not in without]


# the two jobs at the bound: 2^17 ranks each -- tests that are not about the bound leave them out
BOUNDS = ("pair_ranks_large_max", "pair_ranks_large_max_plus_1")
