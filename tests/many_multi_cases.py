"""inputs of the align_many tests for jobs of three and more sequences (RV_MANY_MULTI; tests/test_cpu_many_multi.py checks the
generator itself, tests/test_gpu_many_multi.py uses it): families of k sequences the way the paths through one bubble of a graph
of k genomes look, plus the corner jobs of the eligibility rule and of the index build's size classes.  Deterministic: every job
comes from random.Random(seed).  Built on many_cases.rnd / mutate; the checker is many_cases.oracle_job on the job alone."""
import functools
import random

import many_cases as mc

K_VALUES = (3, 4, 5, 8, 16)
CLASSES = ("snp", "identical", "dropout", "dup", "tandem", "nruns", "lower", "unrelated_one", "len1")
NO_ANCHOR_EXPECTED = ("unrelated_one", "len1")      # one sample shares nothing with the others: no match on every sample
MAX_RANKS = 2048                                    # sum of lengths + k of a job the shared launches take


def ranks(seqs):
    return sum(len(s) for s in seqs) + len(seqs)


def base_length(rng, k):
    """length of a family's common ancestor: every member (a few bases longer at most) fits a job of MAX_RANKS ranks; half of the
    families are small, as most bubbles are"""
    top = (MAX_RANKS - k) // k - 24
    return rng.randint(45, min(top, 150)) if rng.random() < 0.5 or top <= 150 else rng.randint(150, top)


def n_runs(rng, s, most=20):
    a = list(s)
    for _ in range(rng.randint(1, 3)):
        p = rng.randint(0, len(a) - 1)
        for i in range(p, min(len(a), p + rng.randint(1, most))):
            a[i] = "N"
    return "".join(a)


def lower_runs(rng, s):
    a = list(s)
    for _ in range(rng.randint(1, 2)):
        p = rng.randint(0, len(a) - 1)
        for i in range(p, min(len(a), p + rng.randint(1, 25))):
            a[i] = a[i].lower()
    return "".join(a)


def make_family(cls, rng, k):
    L = base_length(rng, k)
    base = mc.rnd(rng, L)
    if cls == "snp":
        return [mc.mutate(rng, base, 0.01) for _ in range(k)]
    if cls == "identical":
        return [base] * k
    if cls == "dropout":                              # one sample is a short piece: it runs out, the children go on with fewer
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
        room = max(2, (L - len(left) - len(right)) // len(unit))
        c0 = rng.randint(2, room)
        return [left + unit * max(1, c0 + rng.choice((-2, -1, 0, 1, 2))) + right for _ in range(k)]
    if cls == "nruns":
        a = n_runs(rng, base)
        return [a] + [mc.mutate(rng, a, 0.005).replace("n", "N") for _ in range(k - 1)]
    if cls == "lower":
        a = lower_runs(rng, base)                    # the family shares its lower-case stretches (a masked repeat); one member may have its own
        fam = [mc.mutate(rng, a, 0.005) for _ in range(k)]
        if rng.random() < 0.3:
            fam[0] = lower_runs(rng, fam[0])
        return fam
    if cls == "unrelated_one":
        fam = [mc.mutate(rng, base, 0.01) for _ in range(k)]
        fam[rng.randrange(k)] = mc.rnd(rng, rng.randint(1, L))
        return fam
    if cls == "len1":
        fam = [mc.mutate(rng, base, 0.01) for _ in range(k)]
        fam[rng.randrange(k)] = rng.choice("ACGT")
        return fam
    raise ValueError(cls)


def class_jobs(per_class, seed=20250301, classes=CLASSES):
    """-> [(class, k, [seq, ..])]: per_class jobs of every class, class by class, k cycling through K_VALUES"""
    out = []
    for cls in classes:
        rng = random.Random(seed * 1000 + CLASSES.index(cls))
        for j in range(per_class):
            k = K_VALUES[j % len(K_VALUES)]
            out.append((cls, k, make_family(cls, rng, k)))
    return out


def split_evenly(total, k):
    return [total // k + (1 if i < total % k else 0) for i in range(k)]


def sized_job(rng, k, nranks, rate=0.01):
    """a family of k sequences with exactly nranks ranks"""
    lens = split_evenly(nranks - k, k)
    base = mc.rnd(rng, max(lens))
    return [mc.mutate(rng, base[:n], rate) for n in lens]


def corner_jobs(seed=5):
    """-> [(name, [seq, ..], taken by the shared launches with RV_MANY_MULTI)]"""
    rng = random.Random(seed)
    return [
        ("three_single_bases", ["A", "C", "A"], True),                        # 6 ranks
        ("sixteen_single_bases", [rng.choice("ACGT") for _ in range(16)], True),      # 32 ranks
        ("ranks_2048", sized_job(rng, 3, 2048), True),
        ("ranks_2049", sized_job(rng, 3, 2049), False),
        ("k17", sized_job(rng, 17, 17 * 40), False),
        ("ranks_512", sized_job(rng, 3, 512), True),                          # the size-class edge of the index build
        ("ranks_513", sized_job(rng, 3, 513), True),
        ("k16_full", sized_job(rng, 16, 2048, 0.002), True),
    ]


def small_jobs(count, seed=9, classes=("snp", "dropout", "identical", "tandem")):
    """jobs of at most ~200 ranks, k = 3 .. 5 (minlength 1 on them gives up to eight anchors per job)"""
    rng = random.Random(seed)
    out = []
    for j in range(count):
        k = (3, 4, 5)[j % 3]
        base = mc.rnd(rng, rng.randint(12, 190 // k))
        cls = classes[j % len(classes)]
        if cls == "snp":
            fam = [mc.mutate(rng, base, 0.05) for _ in range(k)]
        elif cls == "dropout":
            fam = [mc.mutate(rng, base, 0.02) for _ in range(k)]
            fam[rng.randrange(k)] = base[:rng.randint(1, 6)]
        elif cls == "identical":
            fam = [base] * k
        else:
            unit = mc.rnd(rng, rng.randint(1, 4))
            fam = [base[:6] + unit * rng.randint(1, 5) + base[6:12] for _ in range(k)]
        out.append(fam)
    return out


def scale_jobs(count, seed=3):
    """count jobs of k = 3 .. 5 sequences of 40 .. 300 bases, 1 % divergence; the first jobs cover both size classes of the build"""
    rng = random.Random(seed)
    out = []
    for j in range(count):
        k = 3 + j % 3
        L = (40, 300, 100, 160)[j] if j < 4 else rng.randint(40, 300)
        a = mc.rnd(rng, L)
        out.append([mc.mutate(rng, a, 0.01) for _ in range(k)])
    return out


@functools.lru_cache(maxsize=None)
def _oracle(seqs, minl, minn, sa64, arrays):
    return mc.oracle_job(list(seqs), minl, minn, sa64, arrays=arrays)


def oracle_job(seqs, minl=20, minn=2, sa64=False, arrays=False):
    """many_cases.oracle_job, computed once per (job, parameters) and shared between the tests; nobody changes what it returns"""
    return _oracle(tuple(seqs), int(minl), int(minn), bool(sa64), bool(arrays))
