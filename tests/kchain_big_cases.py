"""inputs of the tests of the chaining programme in device memory (csrc/rv_kchain_big.hip): abstract lists rebuilt from the parameters that
tests/golden/kchain_big.json keeps per case (tools/gen_kchain_big_golden.py runs the reference's chain() on them and stores a digest), and the pair
of `chain_recurse`'s test whose top level holds more than 1024 full matches.  Deterministic; T = the tile of the programme."""
import functools
import random

import many_cases as mc

T = 64      # reveal_amd.kchain.KCHAIN_BIG_TILE (tests/test_cpu_kchain_big.py checks it)
MODELS = ("sumofpairs", "star-avg", "star-med")


# ---- the builders of tools/gen_kchain_golden.py, restated so that the tests need nothing but this file (the generator checks them against the originals) ----
def to_records(rng, pts, ls, lens, extra=0):
    k = len(lens)
    begin = [sum(lens[:d]) + d for d in range(k)]
    recs = []
    for pt, l in zip(pts, ls):
        mem = [(d, begin[d] + pt[d]) for d in range(k)]
        rng.shuffle(mem)
        recs.append((l, k, tuple(mem)))
    for _ in range(extra if k > 2 else 0):
        n = rng.randint(2, k - 1)
        sm = rng.sample(range(k), n)
        recs.insert(rng.randrange(len(recs) + 1), (rng.randint(1, 30), n, tuple((d, begin[d] + rng.randrange(lens[d])) for d in sm)))
    return recs


def random_case(rng, k, m, span, noise, lmax=40, equal_l=None):
    cols = [sorted(rng.sample(range(span), m)) for _ in range(k)]
    pts = [[cols[d][i] for d in range(k)] for i in range(m)]
    for d in range(1, k):
        for _ in range(int(noise * m)):
            a, b = rng.randrange(m), rng.randrange(m)
            pts[a][d], pts[b][d] = pts[b][d], pts[a][d]
    ls = [equal_l if equal_l and rng.random() < 0.7 else rng.randint(1, lmax) for _ in range(m)]
    order = list(range(m))
    rng.shuffle(order)
    lens = [span + lmax + rng.randint(0, 30) for _ in range(k)]
    return [tuple(pts[i]) for i in order], [ls[i] for i in order], lens


FNS = dict(to_records=to_records, random_case=random_case)


def tie_points(rng, k, front):
    """tie_case's mirrored pair X, Y (equal lengths, the last coordinates exchanged) in front of a common successor Z, with `front` collinear points in
    front of X: in target order X is point `front`, Y the next, Z the one after"""
    a, b = rng.randint(20, 40), rng.randint(45, 70)
    l = 2 * (b - a) + rng.randint(5, 20)
    pts, ls = [], []
    at = 0
    for _ in range(front):
        at += rng.randint(15, 30)
        pts.append(tuple([at] * k)); ls.append(rng.randint(3, 10))
    o = at + 20
    x, y = [o + a] * k, [o + b] * k
    x[-1], y[-1] = o + b, o + a
    pts += [tuple(x), tuple(y)]; ls += [l, l]
    at = o + b + l + rng.randint(5, 20)
    pts.append(tuple([at] * k)); ls.append(rng.randint(3, 10))
    for _ in range(rng.randint(0, 3)):
        at += rng.randint(15, 30)
        pts.append(tuple([at] * k)); ls.append(rng.randint(3, 10))
    order = list(range(len(pts)))
    rng.shuffle(order)
    return [pts[i] for i in order], [ls[i] for i in order], [at + 40] * k


# where X and Y lie: `front` collinear points in front of X
TIE_PLACEMENTS = {
    "split": T - 1,          # X the last target of tile 0, Y the first of tile 1, Z in Y's tile: one tied offer by push, one by the diagonal
    "tile0": T - 3,          # X, Y and Z in tile 0
    "tile0_push": T - 2,     # X and Y the last two of tile 0, Z the first of tile 1: both tied offers by push
    "tile1": T,              # X, Y and Z in tile 1
    "split12": 2 * T - 1,    # X the last target of tile 1, Y the first of tile 2
}


def p1_stays_points(k):
    """a node (200, 110, ..) with an admissible candidate (0, 100, ..) whose offer loses against p1's, and T fillers in front of it in dimension 0 that
    are not admissible for it (greater in dimension 1): the node is a target of tile 1"""
    if k == 2:
        pts, ls = [(0, 100), (200, 110)], [5, 6]
        pts += [(1 + 2 * i, 121 + 3 * i) for i in range(T)]
    else:
        pts, ls = [(0, 100, 0), (200, 110, 205), (300, 300, 300)], [5, 6, 9]
        pts += [(1 + 2 * i, 121 + 2 * i, 1 + 2 * i) for i in range(T)]
    return pts, ls + [1] * T, [400] * k


def build(case, fns=None):
    """case: an entry of kchain_big.json -> (records, lens)"""
    f = fns or FNS
    rng = random.Random(case["seed"])
    kind, k = case["kind"], case["k"]
    if kind == "random":
        pts, ls, lens = f["random_case"](rng, k, case["m"], case["span"], case["noise"], equal_l=case.get("equal_l"))
        if case.get("run_on"):
            lens = [n + (case["run_on"] if d >= k // 2 else 0) for d, n in enumerate(lens)]
        return f["to_records"](rng, pts, ls, lens, case.get("extra", 0)), lens
    if kind == "tie":
        pts, ls, lens = tie_points(rng, k, case["front"])
        return f["to_records"](rng, pts, ls, lens), lens
    if kind == "p1_stays":
        pts, ls, lens = p1_stays_points(k)
        return f["to_records"](rng, pts, ls, lens), lens
    raise ValueError(kind)


def params(case):
    return dict(maxmums=case["maxmums"], wpen=case["wpen"], wscore=case["wscore"], gcmodel=case["gcmodel"])


def n_kept(case):
    """kept points of the case's list"""
    recs, lens = build(case)
    full = sum(1 for r in recs if r[1] == len(lens))
    return min(full, case["maxmums"]) if case["maxmums"] else full


# ---- chain_recurse: a top level above the cap of the rounds' kernel ----
@functools.lru_cache(maxsize=None)
def recurse_big_input():
    """a pair of about 40 kbp that differs by a SNP every 21 .. 40 bases: more than 1024 full matches of at least 20 bases at the top level"""
    rng = random.Random(4040)
    a = mc.rnd(rng, 40000)
    b = list(a)
    at = rng.randint(21, 40)
    while at < len(b):
        b[at] = rng.choice([c for c in "ACGT" if c != b[at]])
        at += rng.randint(22, 41)
    return (a, "".join(b))
