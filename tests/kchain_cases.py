"""inputs of the kchain tests (tests/test_cpu_kchain.py checks them, tests/test_gpu_kchain.py uses them, tools/gen_kchain_golden.py runs the
reference's chain() on them): the job batches, the parameter sets each batch is chained with, the drivers' inputs, and the list of ONE job alone from
the CPU oracle (getmultimums with minn = k; a pair's getmums records in the multi-MUM shape).  Sequences are str, chained as given.  Deterministic."""
import functools
import hashlib
import json
import random

import many_cases as mc

KS = (2, 3, 8, 32, 64)


def ranks(seqs):
    return sum(len(s) for s in seqs) + len(seqs)


def indel(rng, s, n):
    for _ in range(n):
        p = rng.randrange(1, max(2, len(s) - 1))
        s = s[:p] + mc.rnd(rng, rng.randint(1, 6)) + s[p:] if rng.random() < 0.5 else s[:p] + s[p + rng.randint(1, 6):]
    return s


def family(rng, cls, k, L):
    """k sequences of about L bases of one class"""
    base = mc.rnd(rng, L)
    if cls == "snp":
        return [mc.mutate(rng, base, 0.03) for _ in range(k)]
    if cls == "indel":
        out = [indel(rng, mc.mutate(rng, base, 0.01), 3) for _ in range(k)]
        return [s + mc.rnd(rng, max(0, 10 - len(s))) for s in out]
    if cls == "swap":      # two blocks change places in the last sequence: only one of them chains
        a, b = L // 3, 2 * L // 3
        return [mc.mutate(rng, base, 0.01) for _ in range(k - 1)] + [base[:a // 2] + base[b:] + base[a:b] + base[a // 2:a]]
    if cls == "dup":       # a block twice in the last sequence
        a, b = L // 3, 2 * L // 3
        return [mc.mutate(rng, base, 0.01) for _ in range(k - 1)] + [base[:b] + base[a:b] + base[b:]]
    if cls == "identical":
        return [base] * k
    if cls == "nomatch":
        return [mc.rnd(rng, L, "AC")] + [mc.rnd(rng, L, "GT") for _ in range(k - 1)]
    if cls == "one":       # one full match, nothing else
        x = mc.rnd(rng, 22)
        return [mc.rnd(rng, 4, "AC") + x + mc.rnd(rng, 4, "GT")] + [mc.rnd(rng, 3, "GT") + x + mc.rnd(rng, 5, "AC") for _ in range(k - 1)]
    raise ValueError(cls)


def mirrored(rng, l=24, gap=9):
    """the tie shape in bases: two matches X, Y of equal length mirrored about the diagonal (X Y in the first sequence, Y X in the second) in front of a
    common successor Z: both reach Z with the same score"""
    X, Y, Z = mc.rnd(rng, l), mc.rnd(rng, l), mc.rnd(rng, l + 6)
    f = lambda n, ab: mc.rnd(rng, n, ab)
    return [f(gap, "AC") + X + f(gap, "AC") + Y + f(gap, "AC") + Z + f(5, "AC"), f(gap, "GT") + Y + f(gap, "GT") + X + f(gap, "GT") + Z + f(5, "GT")]


CLASSES = ("snp", "indel", "swap", "dup", "identical", "nomatch", "one")


@functools.lru_cache(maxsize=None)
def mixed_jobs():
    """152 jobs of k = 2, 3, 8, 32, 64 over the seven classes (sequence lengths 10 .. 1000), six mirrored tie shapes, a job of 65 sequences and one
    with a NUL byte (both ordinary), shuffled"""
    rng = random.Random(20261020)
    jobs = []
    for k in KS:
        top = min(980, 2040 // k - 1)
        for cls in CLASSES:
            for _ in range(4):
                L = rng.randint(min(70 if cls in ("swap", "dup") else 10, top), min(top, 740) if cls == "dup" else top)
                jobs.append(family(rng, cls, k, L) if cls != "one" else family(rng, cls, k, 0))
    jobs = [j for j in jobs if ranks(j) <= 2048]
    for _ in range(6):
        jobs.append(mirrored(rng, rng.randint(20, 30), rng.randint(3, 12)))
    jobs.append([mc.mutate(rng, mc.rnd(rng, 28), 0.0) for _ in range(65)])
    nul = mc.rnd(rng, 80)
    jobs.append([nul, nul[:40] + "\0" + nul[41:]])
    rng.shuffle(jobs)
    return tuple(tuple(j) for j in jobs)


@functools.lru_cache(maxsize=None)
def cap_jobs():
    """jobs whose kept list meets the caps: pairs of many short equal-length matches (a cap cuts through equal lengths), a pair with exactly
    RV_KCHAIN_CAP = 4 / 5 full matches under the lowered switch, and k = 8 jobs of many matches"""
    rng = random.Random(77)
    jobs = []
    for n in (4, 5, 9, 30):      # n blocks of 22 bases, a changed base between them: n full matches of length 22
        blocks = [mc.rnd(rng, 22) for _ in range(n)]
        jobs.append(["A".join(blocks), "C".join(blocks)])
        jobs.append(["A".join(blocks), "C".join(blocks), "G".join(blocks)])
    for k in (2, 8):
        jobs.append(family(rng, "snp", k, 2040 // k - 1))
    return tuple(tuple(j) for j in jobs)


def blocks_job(rng, k, n, l=20):
    """k sequences sharing n blocks of l bases, separated by one base that differs from sequence to sequence: n full matches (k <= 4)"""
    blocks = [mc.rnd(rng, l) for _ in range(n)]
    return ["ACGT"[q % 4].join(blocks) for q in range(k)]


@functools.lru_cache(maxsize=None)
def member_jobs():
    """c k at the member cap and just above: 8 sequences x 256 / 257 matches would not fit 2048 ranks, so the cap is met by large-class jobs:
    k = 4, 512 and 513 full matches of length 20 (c k = 2048 and 2052)"""
    rng = random.Random(5)
    return (tuple(blocks_job(rng, 4, 512)), tuple(blocks_job(rng, 4, 513)))


@functools.lru_cache(maxsize=None)
def large_jobs():
    """8 jobs of 2100 .. 30 000 ranks (pairs, k = 3, k = 8) and four small ones"""
    rng = random.Random(31)
    jobs = []
    for k, L in ((2, 1100), (2, 5000), (2, 14000), (3, 700), (3, 4000), (3, 9000), (8, 270), (8, 3700)):
        base = mc.rnd(rng, L)
        jobs.append([indel(rng, mc.mutate(rng, base, 0.02), 4) for _ in range(k)])
    for k in (2, 3, 8, 2):
        jobs.append(family(rng, "indel", k, 150))
    return tuple(tuple(j) for j in jobs)


@functools.lru_cache(maxsize=None)
def wide_score_jobs():
    """a large-class job of k = 8 with one sequence about 60 kbp longer than the rest (its gap costs: 7 pairs x 60 000), and four more large jobs so
    that the class is taken (RV_MANY_SCAN_LARGE_MIN)"""
    rng = random.Random(9)
    base = mc.rnd(rng, 3000)
    fam = [mc.mutate(rng, base, 0.01) for _ in range(8)]
    fam[5] = fam[5][:1500] + mc.rnd(rng, 60000, "AC") + fam[5][1500:]
    jobs = [fam]
    for _ in range(4):
        b = mc.rnd(rng, 1500)
        jobs.append([b, mc.mutate(rng, b, 0.02)])
    return tuple(tuple(j) for j in jobs)


BATCHES = {"mixed": mixed_jobs, "cap": cap_jobs, "members": member_jobs, "large": large_jobs, "wide_score": wide_score_jobs}
P0 = dict(minlength=20, maxmums=0, wpen=1, wscore=1, gcmodel="sumofpairs")


def params(**kw):
    p = dict(P0)
    p.update(kw)
    return p


# the parameter sets each batch is chained with (the golden file holds every pair)
RUNS = {
    "mixed": [params(), params(minlength=5), params(gcmodel="star-avg", maxmums=1), params(gcmodel="star-med", maxmums=3), params(wpen=3), params(wscore=4)],
    "cap": [params(), params(maxmums=1), params(maxmums=3), params(maxmums=4), params(maxmums=3, gcmodel="star-avg")],
    "members": [params()],
    "large": [params(), params(gcmodel="star-med", wpen=3)],
    # (at wpen = 1024 the penalties of wide_score_jobs' first job reach 4.3 x 10^8 -- only the 7 pairs with the long sequence carry its 60 kbp --, which a
    # 32-bit score still holds; the leg at 65536 passes 2^32)
    "wide_score": [params(), params(wpen=1024), params(wpen=65536)],
}


def run_key(batch, p):
    return "%s|minl=%d|maxmums=%d|wpen=%d|wscore=%d|%s" % (batch, p["minlength"], p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"])


def digest(path, end_score):
    """what the golden file keeps of a job's chain: the first 8 digits of a hash of the path (l, positions, score per node) and the end score"""
    flat = [[int(l), [int(x) for x in pos], int(sc)] for l, pos, sc in path]
    return hashlib.sha256(json.dumps([flat, int(end_score)]).encode()).hexdigest()[:8]


# ---- the drivers' inputs ----
@functools.lru_cache(maxsize=None)
def recurse_inputs():
    """-> {name: [seq, ..]}: a pair and a triple of about 5 kbp synthetic genomes with SNPs and indels.  Between the unique stretches lie cassettes
    Q V Q of repeated elements, a base that differs from genome to genome between the elements (so that a maximal match ends with its element): no
    element is unique at the top level, V (whose other copy lies in another gap) is unique in the cassette's gap, and each Q only in the gaps V's
    anchor leaves -- the anchors of depth 1 and depth 2"""
    rng = random.Random(123)
    out = {}
    for name, k in (("pair5k", 2), ("triple5k", 3)):
        genomes = [""] * k

        def put(piece, own):
            for q in range(k):
                genomes[q] += (indel(rng, mc.mutate(rng, piece, 0.03), 1) if own else piece) + "ACG"[q]
        for _ in range(4):
            Q, V = mc.rnd(rng, rng.randint(40, 60)), mc.rnd(rng, rng.randint(40, 60))
            put(mc.rnd(rng, rng.randint(400, 700)), True)
            for piece in (Q, V, Q):
                put(piece, False)
            put(mc.rnd(rng, rng.randint(300, 500)), True)
            put(V, False)
        put(mc.rnd(rng, 300), True)
        out[name] = tuple(genomes)
    return out


RECURSE_PARAMS = dict(minlength=20, minn=2, maxmums=0, wpen=1, wscore=1, gcmodel="sumofpairs")


# ---- the list of one job, alone, from the CPU oracle ----
@functools.lru_cache(maxsize=None)
def oracle_records(seqs, minl):
    """getmultimums(minl, minn = k) of a stand-alone index of the job, as records (l, n, ((sample, pos), ..)) in emission order; a pair's records are
    getmums' in the multi-MUM shape (l, 2, ((0, a), (1, b)))"""
    import bisect
    from helpers import assemble, csr_tuples, oracle
    seqs = list(seqs)
    k = len(seqs)
    T, nsep, _ = assemble(seqs, toupper=False)
    O = oracle(False)
    c = O.construct(T, nsep, k)
    if k == 2:
        l, a, b = O.getmums(c["tbuf"], c["SA"], c["LCP"], nsep, minl)
        return tuple((int(l[i]), 2, ((0, int(a[i])), (bisect.bisect_left(nsep, int(b[i])), int(b[i])))) for i in range(len(l)))
    return tuple(csr_tuples(*O.getmultimums(c["tbuf"], c["SA"], c["LCP"], c["SO"], nsep, k, minl, k)))
