"""inputs of the align_many tests for pair jobs above 2048 ranks (RV_MANY_LARGE; tests/test_cpu_many_large.py checks the generator itself,
tests/test_gpu_many_large.py uses it): the classes of many_cases scaled up to sequences of about 1 .. 3 kbp, and the corner cases of the
index build in device memory -- the first size above the leaf kernel's, ties through '$' over thousands of characters, alleles of 10 kbp,
and one job whose ranks do not fit 16 bits.  Deterministic: every job comes from random.Random(seed)."""
import random

from many_cases import mutate, oracle_job, rnd  # noqa: F401  (oracle_job: for the tests that import this module)

CLASSES = ("snp", "indel", "identical", "unrelated", "homopolymer", "tandem", "nruns", "lower", "tails", "onebase")
LMIN, LMAX = 1060, 2990                         # length of the first sequence: every job stays within 2049 .. 6100 ranks
RANKS_MIN, RANKS_MAX = 2049, 6100


def make_large_pair(cls, rng):
    L = rng.randint(LMIN, LMAX)
    if cls == "snp":
        a = rnd(rng, L)
        return a, mutate(rng, a, 0.01)
    if cls == "indel":
        a = rnd(rng, L)
        b = a
        for _ in range(rng.randint(1, 3)):
            p = rng.randint(0, len(b) - 1)
            k = rng.randint(1, 10)
            b = b[:p] + (rnd(rng, k) if rng.random() < 0.5 else "") + b[p + (k if rng.random() < 0.5 else 0):]
        return a, b
    if cls == "identical":
        a = rnd(rng, L)
        return a, a
    if cls == "unrelated":
        return rnd(rng, L), rnd(rng, rng.randint(LMIN, LMAX))
    if cls == "homopolymer":
        if rng.random() < 0.4:                       # the bare case: A^n against A^(n-1), every suffix ties inside its own sequence
            return "A" * L, "A" * (L - 1)
        left, right = rnd(rng, rng.randint(25, 40)), rnd(rng, rng.randint(25, 40))
        c = rng.choice("ACGT")
        n = L - len(left) - len(right)
        return left + c * n + right, left + c * (n - 1) + right
    if cls == "tandem":
        unit = rnd(rng, rng.randint(2, 7))
        ca = (L - 80) // len(unit)
        cb = ca + rng.choice((-2, -1, 1, 2))
        if rng.random() < 0.4:
            return unit * ca, unit * cb
        left, right = rnd(rng, rng.randint(25, 40)), rnd(rng, rng.randint(25, 40))
        return left + unit * ca + right, left + unit * cb + right
    if cls == "nruns":
        a = list(rnd(rng, L))
        for _ in range(rng.randint(1, 6)):
            p = rng.randint(0, len(a) - 1)
            for i in range(p, min(len(a), p + rng.randint(1, 30))):
                a[i] = "N"
        a = "".join(a)
        return a, mutate(rng, a, 0.005).replace("n", "N")
    if cls == "lower":
        a = rnd(rng, L)
        b = list(mutate(rng, a, 0.01))
        a = list(a)
        for s in (a, b):
            for _ in range(rng.randint(1, 6)):
                p = rng.randint(0, len(s) - 1)
                for i in range(p, min(len(s), p + rng.randint(1, 40))):
                    s[i] = s[i].lower()
        return "".join(a), "".join(b)
    if cls == "tails":
        s = rnd(rng, max(L, 1150) - 100)
        x, y = rnd(rng, rng.randint(1, 150)), rnd(rng, rng.randint(1, 150))
        k = rng.randint(0, 2)
        if k == 0:
            return x + s, y + s                      # equal tails: the suffixes of s tie up to and including the '$'
        if k == 1:
            return s + x, s + y                      # equal heads
        return s, x + s                              # one allele is a suffix of the other
    if cls == "onebase":
        a = rnd(rng, L)
        p = rng.randint(0, len(a) - 1)
        return a, a[:p] + rng.choice([c for c in "ACGT" if c != a[p]]) + a[p + 1:]
    raise ValueError(cls)


def large_class_jobs(per_class, seed=20250301):
    """-> [(class, (a, b))]: per_class pair jobs of every class, class by class, each of RANKS_MIN .. RANKS_MAX ranks"""
    out = []
    for ci, cls in enumerate(CLASSES):
        rng = random.Random(seed * 1000 + ci)
        for _ in range(per_class):
            out.append((cls, make_large_pair(cls, rng)))
    return out


CORNER_RANKS = (2049, 2048, 3001, 4196, 4003, 20000, 20000, 80002)


def corner_jobs(seed=31):
    """-> [(a, b)] with CORNER_RANKS ranks: the first size above the leaf kernel's and the last one within it, a bare homopolymer and a bare
    tandem repeat, a one-base second sequence, alleles of 9 999 bases (1 % apart, and identical), and last a job of 80 002 ranks"""
    rng = random.Random(seed)
    x = rnd(rng, 1024)
    u = "ACG"
    out = [(x[:1024], x[:1023]), (x[:1024], x[:1022]), ("A" * 1500, "A" * 1499), (u * 700, u * 698), (rnd(rng, 4000), "A")]
    a = rnd(rng, 9999)
    out.append((a, mutate(rng, a, 0.01)))
    a = rnd(rng, 9999)
    out.append((a, a))
    a = rnd(rng, 40000)
    out.append((a, mutate(rng, a, 0.01)))
    return out
