"""inputs of the align_many tests for jobs of three and more sequences above 2048 ranks (RV_MANY_LARGE_MULTI; tests/test_cpu_many_large_multi.py
checks the generator itself, tests/test_gpu_many_large_multi.py uses it): the families of many_multi_cases scaled up to 2049 .. 6100 ranks, and the
corner cases of the sample-major rounds -- the first size above the leaf kernel's, the widest job, a one-base sequence, ties through '$' over
thousands of characters among three suffixes, alleles of 6.7 kbp, and one job whose ranks do not fit 16 bits.  Deterministic: every job comes
from random.Random(seed).  The checker is many_multi_cases.oracle_job on the job alone."""
import random

import many_cases as mc
import many_multi_cases as mm
from many_multi_cases import oracle_job, ranks, sized_job  # noqa: F401  (for the tests that import this module)

K_VALUES = mm.K_VALUES                               # (3, 4, 5, 8, 16)
CLASSES = ("snp", "identical", "dropout", "dup", "tandem", "nruns", "lower", "unrelated_one")
NO_ANCHOR_EXPECTED = ("unrelated_one",)             # one sample shares nothing with the others: no match on every sample
RANKS_MIN, RANKS_MAX = 2049, 6100


def base_length(rng, k):
    """length of a family's common ancestor: the job stays within RANKS_MIN .. RANKS_MAX ranks even when one member is a short piece
    (dropout, unrelated_one) or a few repeat units longer (tandem)"""
    return rng.randint((RANKS_MIN - k) // (k - 1) + 45, (RANKS_MAX - k) // k - 24)


def make_large_family(cls, rng, k):
    """many_multi_cases.make_family at these sizes (the same classes from the same pieces; N runs and lower-case stretches stay as short as
    there, so a family keeps long matches between them)"""
    L = base_length(rng, k)
    base = mc.rnd(rng, L)
    if cls == "snp":
        return [mc.mutate(rng, base, 0.01) for _ in range(k)]
    if cls == "identical":                           # ties through '$' over the whole allele among k suffixes
        return [base] * k
    if cls == "dropout":                             # one sample is a short piece: it runs out, the children go on with fewer
        fam = [mc.mutate(rng, base, 0.005) for _ in range(k)]
        n = rng.randint(21, 40)
        p = rng.randint(0, L - n)
        fam[rng.randrange(k)] = base[p:p + n]
        return fam
    if cls == "dup":
        fam = [mc.mutate(rng, base, 0.03) for _ in range(k)]
        i, j = rng.sample(range(k), 2)
        fam[j] = fam[i]
        return fam
    if cls == "tandem":
        unit = mc.rnd(rng, rng.randint(2, 7))
        left, right = mc.rnd(rng, rng.randint(25, 40)), mc.rnd(rng, rng.randint(25, 40))
        c0 = (L - len(left) - len(right)) // len(unit) - 2
        return [left + unit * (c0 + rng.choice((-2, -1, 0, 1, 2))) + right for _ in range(k)]
    if cls == "nruns":
        a = mm.n_runs(rng, base)
        return [a] + [mc.mutate(rng, a, 0.005).replace("n", "N") for _ in range(k - 1)]
    if cls == "lower":
        a = mm.lower_runs(rng, base)
        fam = [mc.mutate(rng, a, 0.005) for _ in range(k)]
        if rng.random() < 0.3:
            fam[0] = mm.lower_runs(rng, fam[0])
        return fam
    if cls == "unrelated_one":
        fam = [mc.mutate(rng, base, 0.01) for _ in range(k)]
        fam[rng.randrange(k)] = mc.rnd(rng, rng.randint(1, L))
        return fam
    raise ValueError(cls)


def class_jobs(per_class, seed=20250915, classes=CLASSES):
    """-> [(class, k, [seq, ..])]: per_class jobs of every class, class by class, k cycling through K_VALUES over the whole list"""
    out = []
    for cls in classes:
        rng = random.Random(seed * 1000 + CLASSES.index(cls))
        for _ in range(per_class):
            k = K_VALUES[len(out) % len(K_VALUES)]
            out.append((cls, k, make_large_family(cls, rng, k)))
    return out


CORNER_NAMES = ("ranks_2049", "ranks_2048", "k16_2064", "one_base", "homopolymer", "tandem", "three_6666", "three_22000")
CORNER_RANKS = (2049, 2048, 2064, 3004, 3000, 2694, 20001, 66003)


def corner_jobs(seed=41):
    """-> [[seq, ..]] named CORNER_NAMES with CORNER_RANKS ranks: k = 3 with the first size above the leaf kernel's and its neighbour within it
    (that one is not of this class), k = 16 with 16 x 128 + 16 ranks, a job one of whose sequences is a single base, a bare homopolymer family
    A^n, A^(n-1), A^(n-2), a bare tandem family, 3 x 6666 bases 1 % apart, and last 3 x 22 000 bases"""
    rng = random.Random(seed)
    out = [sized_job(rng, 3, 2049), sized_job(rng, 3, 2048), sized_job(rng, 16, 2064, 0.002)]
    a = mc.rnd(rng, 1500)
    out.append([a, "A", mc.mutate(rng, a, 0.01)])
    out.append(["A" * 1000, "A" * 999, "A" * 998])
    out.append(["ACG" * 300, "ACG" * 299, "ACG" * 298])
    a = mc.rnd(rng, 6666)
    out.append([mc.mutate(rng, a, 0.01) for _ in range(3)])
    a = mc.rnd(rng, 22000)
    out.append([mc.mutate(rng, a, 0.01) for _ in range(3)])
    return out


def sized_jobs(count, k_values=(3, 4, 5, 8, 16), lo=2049, hi=2300, seed=17):
    """count families of lo .. hi ranks, 1 % apart, k cycling through k_values (sized_job)"""
    rng = random.Random(seed)
    return [sized_job(rng, k_values[j % len(k_values)], rng.randint(lo, hi)) for j in range(count)]
