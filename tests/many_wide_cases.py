"""inputs of the align_many tests for jobs of 17 .. 64 sequences (RV_MANY_WIDE; tests/test_cpu_many_wide.py checks the generator itself,
tests/test_gpu_many_wide.py uses it): families of k sequences the way a bubble of k haplotypes looks -- one ancestor, one to three variant
sites, every site substituted in a subset of the members -- plus the classes of many_multi_cases at the member lengths a job of k sequences
leaves (31 bases at k = 64 and 2048 ranks), and the corner jobs of the eligibility rule.  A per-member mutation rate is the wrong model here:
among 64 members almost every window carries a difference somewhere, the picker (a match on EVERY sample) finds nothing, and a test passes
while it tests nothing.  Deterministic: every job comes from random.Random(seed).  The checker is many_multi_cases.oracle_job on the job alone."""
import random

import many_cases as mc
import many_multi_cases as mm
from many_multi_cases import oracle_job, ranks  # noqa: F401  (for the tests that import this module)

K_VALUES = (17, 24, 32, 33, 48, 64)      # 17: the first lane above 16, sample id bit 4; 32 | 33: either side of a 32-bit census; 64: lane 63
CLASSES = ("sites", "identical", "dropout", "tandem", "nruns", "lower", "len1", "unrelated_one")
NO_ANCHOR_EXPECTED = ("len1", "unrelated_one")      # one sample shares nothing with the others: no match on every sample
MAX_RANKS = 2048                                    # sum of lengths + k of a small job
LARGE_RANKS = (2049, 6000)                          # ... of the large jobs of this file


def top_length(k, max_ranks=MAX_RANKS):
    """the longest member with which k equally long members stay within max_ranks ranks"""
    return (max_ranks - k) // k


def base_length(rng, k, lo=None, hi=None):
    top = top_length(k) if hi is None else hi
    return rng.randint(min(25, top) if lo is None else lo, top)


def with_sites(rng, base, k, most=3):
    """k copies of base; 1 .. most variant sites, each substituted (one other base) in a random non-empty proper subset of the members"""
    fam = [list(base) for _ in range(k)]
    for p in rng.sample(range(len(base)), min(len(base), rng.randint(1, most))):
        alt = rng.choice([c for c in "ACGT" if c != base[p].upper()])
        for i in rng.sample(range(k), rng.randint(1, k - 1)):
            fam[i][p] = alt
    return ["".join(s) for s in fam]


def make_family(cls, rng, k, lo=None, hi=None):
    """a family of class cls: members of at most `hi` bases (default: what keeps the job within MAX_RANKS ranks)"""
    top = top_length(k) if hi is None else hi
    L = base_length(rng, k, lo, hi)
    base = mc.rnd(rng, L)
    if cls == "sites":
        return with_sites(rng, base, k)
    if cls == "identical":                            # k suffixes tie through '$' at every position
        return [base] * k
    if cls == "dropout":                              # one member is a short piece at an end: it runs out, the children go on with k - 1
        fam = with_sites(rng, base, k, most=1)
        n = rng.randint(min(12, L), max(min(12, L), L // 2))
        fam[rng.randrange(k)] = base[:n] if rng.random() < 0.5 else base[L - n:]
        return fam
    if cls == "tandem":
        unit = mc.rnd(rng, rng.randint(2, 4))
        e = max(1, min(8, top // 4))                  # (flanks that leave room for the unit in the shortest members this file makes)
        left, right = mc.rnd(rng, rng.randint(min(4, e), e)), mc.rnd(rng, rng.randint(min(4, e), e))
        room = max(1, (top - len(left) - len(right)) // len(unit))      # copies of the unit the longest member may hold
        c0 = rng.randint(1, room)
        return [left + unit * min(room, max(1, c0 + rng.choice((-2, -1, 0, 1, 2)))) + right for _ in range(k)]
    if cls == "nruns":
        return with_sites(rng, mm.n_runs(rng, base, most=max(1, L // 6)), k)
    if cls == "lower":
        fam = with_sites(rng, mm.lower_runs(rng, base), k)      # the family shares its lower-case stretches; one member may have its own
        if rng.random() < 0.3:
            fam[0] = mm.lower_runs(rng, fam[0])
        return fam
    if cls == "len1":
        fam = with_sites(rng, base, k)
        fam[rng.randrange(k)] = rng.choice("ACGT")
        return fam
    if cls == "unrelated_one":
        fam = with_sites(rng, base, k)
        fam[rng.randrange(k)] = mc.rnd(rng, rng.randint(1, L))
        return fam
    raise ValueError(cls)


def sites_jobs(per_k, seed=20261019, k_values=K_VALUES):
    """-> [(k, [seq, ..])]: per_k jobs of class "sites" for every k, k by k"""
    out = []
    for k in k_values:
        rng = random.Random(seed * 1000 + k)
        out += [(k, make_family("sites", rng, k)) for _ in range(per_k)]
    return out


def class_jobs(per_k, seed=20261020, classes=CLASSES, k_values=K_VALUES):
    """-> [(class, k, [seq, ..])]: per_k jobs for every k, the classes cycling, k by k; every job at most MAX_RANKS ranks"""
    out = []
    for k in k_values:
        rng = random.Random(seed * 1000 + k)
        for j in range(per_k):
            cls = classes[j % len(classes)]
            out.append((cls, k, make_family(cls, rng, k)))
    return out


def short_jobs(per_k, max_ranks=600, seed=8, k_values=(17, 33, 64), classes=("sites", "dropout", "identical", "tandem")):
    """jobs of at most about max_ranks ranks (minlength 1 and 5 on them: several anchors a job)"""
    out = []
    for k in k_values:
        rng = random.Random(seed * 1000 + k)
        top = max(3, top_length(k, max_ranks))
        out += [make_family(classes[j % len(classes)], rng, k, lo=min(top, 6), hi=top) for j in range(per_k)]
    return out


def large_jobs(per_k, seed=12, k_values=(17, 33, 64), classes=("sites", "identical", "dropout", "lower")):
    """-> [(class, k, [seq, ..])] of LARGE_RANKS[0] .. LARGE_RANKS[1] ranks: the families above with longer members"""
    out = []
    for k in k_values:
        rng = random.Random(seed * 1000 + k)
        lo, hi = (LARGE_RANKS[0] - k) // (k - 1) + 14, top_length(k, LARGE_RANKS[1])      # (a dropout member is at least 12 bases)
        for j in range(per_k):
            cls = classes[j % len(classes)]
            out.append((cls, k, make_family(cls, rng, k, lo=lo, hi=hi)))
    return out


def scale_jobs(count, seed=3):
    """count "sites" jobs, k cycling through K_VALUES"""
    rng = random.Random(seed)
    return [make_family("sites", rng, K_VALUES[j % len(K_VALUES)]) for j in range(count)]


CORNER_NAMES = ("k17_single_bases", "k64_single_bases", "k17", "k64_full", "k64_2049", "k65", "k16")


def corner_jobs(seed=6):
    """-> [(name, [seq, ..], class)], class one of "small" (shared with RV_MANY_WIDE), "large" (shared in a call with at least
    RV_MANY_WIDE_LARGE_MIN such jobs), "never" (more than 64 sequences) and "other" (16 sequences: where it went before)"""
    rng = random.Random(seed)
    k17 = dict((n, s) for n, s, _ in mm.corner_jobs())["k17"]                       # 17 x 40 ranks: the job many_multi_cases pins as ordinary
    full = with_sites(rng, mc.rnd(rng, 31), 64)                                    # 64 x 31 bases: 2048 ranks
    over = with_sites(rng, mc.rnd(rng, 31), 64)
    over[rng.randrange(64)] += "A"                                                 # 2049 ranks
    return [
        ("k17_single_bases", [rng.choice("ACGT") for _ in range(17)], "small"),    # 34 ranks
        ("k64_single_bases", [rng.choice("ACGT") for _ in range(64)], "small"),    # 128 ranks
        ("k17", k17, "small"),
        ("k64_full", full, "small"),
        ("k64_2049", over, "large"),
        ("k65", with_sites(rng, mc.rnd(rng, 20), 65), "never"),
        ("k16", with_sites(rng, mc.rnd(rng, 60), 16), "other"),
    ]
