"""inputs of the align_many tests (tests/test_cpu_many.py checks the generator itself, tests/test_gpu_many.py uses it): pair jobs the
way bubbles of a graph look -- near-identical alleles, repeats, N runs -- plus the corner cases of the shared index build (ties through
'$', length-1 sequences).  Deterministic: every job comes from random.Random(seed)."""
import random

CLASSES = ("snp", "indel", "identical", "unrelated", "homopolymer", "tandem", "nruns", "lower", "tails", "len1", "onebase")
NO_ANCHOR_EXPECTED = ("unrelated", "len1")      # the only classes in which most jobs have nothing to anchor at minlength 20
MAXL = 990                                      # longest sequence of a class job: la + lb + 2 stays below 2048 with a few inserted bases


def rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, rate):
    out = list(s)
    for i in range(len(out)):
        if rng.random() < rate:
            out[i] = rng.choice([c for c in "ACGT" if c != out[i]])
    return "".join(out)


def length(rng):
    """1 .. MAXL, half of them below 150 (most bubbles are small)"""
    return rng.randint(1, 150) if rng.random() < 0.5 else rng.randint(150, MAXL)


def make_pair(cls, rng):
    L = length(rng)
    if cls == "snp":
        a = rnd(rng, max(L, 30))
        return a, mutate(rng, a, 0.01)
    if cls == "indel":
        a = rnd(rng, max(L, 60))
        b = a
        for _ in range(rng.randint(1, 3)):
            p = rng.randint(0, len(b) - 1)
            k = rng.randint(1, 10)
            b = b[:p] + (rnd(rng, k) if rng.random() < 0.5 else "") + b[p + (k if rng.random() < 0.5 else 0):]
        return a, (b[:MAXL + 20] or "A")
    if cls == "identical":
        a = rnd(rng, max(L, 20))
        return a, a
    if cls == "unrelated":
        return rnd(rng, L), rnd(rng, length(rng))
    if cls == "homopolymer":
        n = max(L, 2)
        if rng.random() < 0.4:                       # the bare case: A^n against A^(n-1), every suffix ties inside its own sequence
            return "A" * n, "A" * (n - 1)
        n = min(n, MAXL - 80)
        left, right = rnd(rng, rng.randint(25, 40)), rnd(rng, rng.randint(25, 40))
        c = rng.choice("ACGT")
        return left + c * n + right, left + c * (n - 1) + right
    if cls == "tandem":
        unit = rnd(rng, rng.randint(2, 7))
        ca = rng.randint(2, max(2, min(L, MAXL - 100) // len(unit)))
        cb = max(1, ca + rng.choice((-2, -1, 1, 2)))
        if rng.random() < 0.4:
            return unit * ca, unit * cb
        left, right = rnd(rng, rng.randint(25, 40)), rnd(rng, rng.randint(25, 40))
        return left + unit * ca + right, left + unit * cb + right
    if cls == "nruns":
        a = list(rnd(rng, max(L, 80)))
        for _ in range(rng.randint(1, 3)):
            p = rng.randint(0, len(a) - 1)
            for i in range(p, min(len(a), p + rng.randint(1, 30))):
                a[i] = "N"
        a = "".join(a)
        return a, mutate(rng, a, 0.005).replace("n", "N")
    if cls == "lower":
        a = rnd(rng, max(L, 80))
        b = list(mutate(rng, a, 0.01))
        a = list(a)
        for s in (a, b):
            for _ in range(rng.randint(1, 3)):
                p = rng.randint(0, len(s) - 1)
                for i in range(p, min(len(s), p + rng.randint(1, 40))):
                    s[i] = s[i].lower()
        return "".join(a), "".join(b)
    if cls == "tails":
        s = rnd(rng, max(min(L, MAXL - 300), 25))
        x, y = rnd(rng, rng.randint(1, 150)), rnd(rng, rng.randint(1, 150))
        k = rng.randint(0, 2)
        if k == 0:
            return x + s, y + s                      # equal tails: the suffixes of s tie up to and including the '$'
        if k == 1:
            return s + x, s + y                      # equal heads
        return s, x + s                              # one allele is a suffix of the other
    if cls == "len1":
        k = rng.randint(0, 3)
        if k == 0:
            return rng.choice("ACGTN"), rng.choice("ACGTN")
        if k == 1:
            return rng.choice("ACGT"), rnd(rng, L)
        if k == 2:
            return rnd(rng, L), rng.choice("ACGT")
        return "A", "A"
    if cls == "onebase":
        a = rnd(rng, max(L, 45))
        p = rng.randint(0, len(a) - 1)
        return a, a[:p] + rng.choice([c for c in "ACGT" if c != a[p]]) + a[p + 1:]
    raise ValueError(cls)


def oracle_job(seqs, minl=20, minn=2, sa64=False, arrays=False):
    """the reference result of ONE job, alone: assemble + construct + align_bench of the CPU oracle (pinned to the reference's C)
    -> (sorted anchors [(l, (pos, ..))], final text bytes[, SA, LCP])"""
    from helpers import assemble, oracle
    T, nsep, nodes = assemble(list(seqs), toupper=False)
    O = oracle(sa64)
    c = O.construct(T, nsep, len(seqs))
    sa, lcp = (c["SA"].copy(), c["LCP"].copy()) if arrays else (None, None)
    ref = O.align_bench(c, nodes, minl, minn, anchor_cap=len(T) + 16)
    rl, rn, roff, rpos = ref["anchors"]
    anchors = sorted((int(rl[k]), tuple(int(x) for x in rpos[roff[k]:roff[k + 1]])) for k in range(len(rl)))
    return (anchors, ref["T"], sa, lcp) if arrays else (anchors, ref["T"])


def class_jobs(per_class, seed=20240611):
    """-> [(class, (a, b))]: per_class jobs of every class, class by class"""
    out = []
    for ci, cls in enumerate(CLASSES):
        rng = random.Random(seed * 1000 + ci)
        for _ in range(per_class):
            out.append((cls, make_pair(cls, rng)))
    return out


def big_pairs(count, seed=7):
    """pair jobs above 2048 ranks (the ordinary path)"""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        a = rnd(rng, rng.randint(1024, 3000))
        out.append((a, mutate(rng, a, 0.01)))
    return out


def multi_jobs(seed=11):
    """jobs of three and of five sequences (the ordinary path): three of three, two of five"""
    rng = random.Random(seed)
    out = []
    for k in (3, 3, 3, 5, 5):
        base = rnd(rng, rng.randint(100, 600))
        out.append([mutate(rng, base, 0.01) for _ in range(k)])
    return out


def scale_jobs(count, seed=3):
    """count pair jobs of 2 x (40 .. 300) bases, 1 % divergence; the first jobs cover both size classes of the index build"""
    rng = random.Random(seed)
    out = []
    for j in range(count):
        L = (40, 300, 100, 256)[j] if j < 4 else rng.randint(40, 300)
        a = rnd(rng, L)
        out.append((a, mutate(rng, a, 0.01)))
    return out
