"""shared cases of the getblocks tests (tests/test_cpu_blocks.py, tests/test_gpu_blocks.py) and of tools/gen_blocks_golden.py, which runs the
reference's own addctginfo + clustermumsbydiagonal on them and writes tests/golden/blocks.json.  Everything here is deterministic.

  oracle lists     MUMs of the CPU oracle on golden FASTA pairs and on one synthetic reference / draft assembly, in both orientations
  abstract lists   hand-made records plus ranges: the boundaries of the rule, the record counts round the kernels' workgroup size, one
                   cluster across every workgroup, coordinates that need the two-pass sort
"""
import hashlib
import json
import os
import random

from helpers import GOLD, assemble, fa, oracle

DEFAULTS = dict(minlength=20, cluster=True, maxdist=30, minclustsize=50)      # `reveal transform`'s own

# variants every fixture pair runs under, both orientations: name -> what differs from DEFAULTS
VARIANTS = {
    "defaults": {},
    "nocluster": dict(cluster=False),
    "maxdist1": dict(maxdist=1),
    "maxdist0": dict(maxdist=0),
    "minclust0": dict(minclustsize=0),
    "minclust_huge": dict(minclustsize=10 ** 9),      # above every score: no block
    "minlength_huge": dict(minlength=10 ** 6),        # above every LCP value: no MUM, no block, no error
}
FIXTURES = {"1a+1b": ("1a", "1b"), "1a+1brc": ("1a", "1brc")}


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def oracle_mums(inputs, minlength, rc, sa64=False):
    """-> ([(l, (a, b), rc)] as index.getmums gives them after construct(rc), ranges of every sequence in order of addition)"""
    T, nsep, nodes = assemble(inputs)
    O = oracle(sa64)
    tb = O.textbuf(T)
    if rc:
        O.revcomp(tb[nsep[0]:len(T)])
    SA = O.suffix_array(tb)
    LCP = O.compute_lcp(tb, SA, O.inverse(SA))
    l, a, b = O.getmums(tb, SA, LCP, nsep, minlength, rc=1 if rc else 0, nT=len(T))
    return [(int(l[k]), (int(a[k]), int(b[k])), 1 if rc else 0) for k in range(len(l))], nodes


def keys_unique(mums, rc):
    """the claim behind the rule's total order: no two MUMs share the reference's sort key"""
    if rc:
        keys = [(a + b + l, a - (b + l)) for l, (a, b), *_ in mums]
    else:
        keys = [(a - b, a + b) for l, (a, b), *_ in mums]
    return len(set(keys)) == len(keys) and len({b for _, (_, b), *_ in mums}) == len(mums)


# ---- the synthetic assembly: a reference of two sequences, four contigs cut from it (two reverse-complemented, one joining both reference
# sequences) and one contig below minctglength
MULTI = dict(minlength=10, cluster=True, maxdist=30, minclustsize=30)
MULTI_MINCTG = 200


def _comp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def _mutate(rng, s, rate):
    out = list(s)
    for k in range(len(out)):
        if rng.random() < rate:
            out[k] = rng.choice([c for c in "ACGT" if c != out[k]])
    return "".join(out)


def multi_case():
    """-> (reference sequences, contigs): the last contig is shorter than MULTI_MINCTG and must be skipped"""
    rng = random.Random(20261020)
    r0 = "".join(rng.choice("ACGT") for _ in range(1500))
    r1 = "".join(rng.choice("ACGT") for _ in range(900))
    contigs = [
        _mutate(rng, r0[100:700], 0.03),
        _comp(_mutate(rng, r0[750:1400], 0.04)),
        _mutate(rng, r0[1380:1500] + r1[0:300], 0.05),                 # joins the two reference sequences
        _comp(_mutate(rng, r1[350:850], 0.03)),
        r1[860:900] + "".join(rng.choice("ACGT") for _ in range(60)),      # 100 bases: below minctglength
    ]
    return [r0, r1], contigs


def multi_inputs():
    ref, ctgs = multi_case()
    return [ref, [c for c in ctgs if len(c) >= MULTI_MINCTG]]


# ---- abstract lists
RANGES4 = [(0, 999), (1000, 1999), (2000, 2999), (3000, 3999)]      # two reference sequences, two contigs; '$' at 999, 1999, 2999, 3999


def _walk(rng, n, o, R, Q, base=0):
    """n records on a handful of (anti-)diagonals between a reference [base, base + R) and contigs [base + R, base + R + Q): gaps of 0 .. 60 and
    lengths of 5 .. 40, so that with maxdist 30 some neighbours merge and some do not; no two records share a key"""
    recs, used = [], set()
    while len(recs) < n:
        while True:
            off = rng.randrange(-R // 2, Q - R // 2)
            if off not in used:
                used.add(off)
                break
        a = rng.randrange(0, 50)
        while len(recs) < n:
            l = rng.randint(5, 40)
            b = (a + off) if not o else (Q + off - a - l)      # o = 1: a + b + l constant
            if a + l >= R:
                break
            if 0 <= b and b + l < Q:
                recs.append((l, (base + a, base + R + b), o))
            a += l + rng.randint(0, 60)
    rng.shuffle(recs)
    return recs


def _ranges(R, Q, base=0):
    return [(base, base + R // 3), (base + R // 3 + 1, base + R - 1), (base + R, base + R + Q // 2), (base + R + Q // 2 + 1, base + R + Q - 1)]


def abstract_cases():
    """name -> dict(mums, ranges, rc, kw): kw as blocks_python takes it"""
    C = {}

    def add(name, mums, ranges=RANGES4, rc=0, **kw):
        C[name] = dict(mums=[(l, (a, b), rc) for l, (a, b), *_ in mums], ranges=ranges, rc=rc, kw=dict(dict(cluster=True, maxdist=30, minclustsize=50), **kw))

    add("dist_eq_maxdist", [(40, (10, 2010)), (40, (80, 2080))], minclustsize=0)                      # 80 - 50 = 30: not merged
    add("dist_maxdist_minus1", [(40, (10, 2010)), (40, (79, 2079))], minclustsize=0)                  # 29: merged
    add("score_eq_min", [(25, (10, 2010)), (25, (40, 2040))])                                         # 50: kept
    add("score_min_minus1", [(25, (10, 2010)), (24, (40, 2040))])                                     # 49: dropped
    add("split_contigs", [(30, (100, 2960)), (30, (145, 3005))], minclustsize=0)                      # one diagonal, b in two contigs
    add("split_refs", [(30, (960, 2060)), (30, (1005, 2105))], minclustsize=0)                        # one diagonal, a in two reference sequences
    add("at_end_plus_1", [(10, (999, 2999)), (10, (1000, 3000)), (10, (1999, 3999)), (10, (0, 2000)), (10, (1011, 3011))], minclustsize=0)
    add("rc_pair", [(20, (100, 2500)), (20, (130, 2470))], rc=1, minclustsize=0)                      # merged: s2 from the last, e2 from the first
    add("rc_three", [(20, (100, 2500)), (15, (130, 2475)), (20, (200, 2400)), (30, (300, 2900))], rc=1, minclustsize=0)
    add("rc_split_contigs", [(20, (100, 3010)), (20, (130, 2980))], rc=1, minclustsize=0)
    add("overlap", [(20, (100, 2100)), (20, (110, 2110))])                                            # error
    add("overlap_other_ids", [(20, (990, 2100)), (20, (1000, 2110))], minclustsize=0)                 # the same overlap across two reference sequences: no error
    add("empty", [])
    for n in (1, 2, 255, 256, 257, 5000):
        for o in (0, 1):
            rng = random.Random(1000 * n + o)
            add("walk_%d_o%d" % (n, o), _walk(rng, n, o, 40000, 60000), _ranges(40000, 60000), rc=o, minclustsize=40)
    add("walk_5000_nocluster", _walk(random.Random(7), 5000, 0, 40000, 60000), _ranges(40000, 60000), cluster=False)
    one = [(10, (15 * k, 100001 + 15 * k)) for k in range(5000)]
    random.Random(11).shuffle(one)
    add("one_diagonal_merged", one, [(0, 100000), (100001, 200001)])                                  # one block over every workgroup and sort tile
    add("one_diagonal_maxdist0", one, [(0, 100000), (100001, 200001)], maxdist=0, minclustsize=0)     # 5000 blocks
    base = 1 << 40                                                                                    # first component and a do not fit one 64-bit key
    for o in (0, 1):
        add("wide_o%d" % o, _walk(random.Random(50 + o), 600, o, 40000, 60000, base), [(0, base - 1)] + _ranges(40000, 60000, base), rc=o, minclustsize=40)
    return C


def digest(blocks):
    return hashlib.sha256(json.dumps([list(map(int, b)) for b in blocks]).encode()).hexdigest()


def golden():
    with open(os.path.join(GOLD, "blocks.json")) as f:
        return json.load(f)


def matches_golden(blocks, rec):
    """a golden record holds the block list, or for a long one its length and digest"""
    if "blocks" in rec:
        return [list(map(int, b)) for b in blocks] == rec["blocks"]
    return len(blocks) == rec["count"] and digest(blocks) == rec["sha256"]


def fixture_inputs(name):
    return fa(*FIXTURES[name])
