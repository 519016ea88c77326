"""shared cases of the glocal chain tests (tests/test_cpu_glocal.py, tests/test_gpu_glocal.py) and of tools/gen_glocal_golden.py, which runs the
reference's own glocalchain (useheap=False) on them, one pass per axis and the two loops of transform.py:307-356, and writes tests/golden/glocal.json
(a chain = the indices of the kept input blocks).  Everything here is seeded and deterministic.  Two reference sequences and three contigs; no two
blocks of a list are equal (the reference keys a dictionary by the block).
"""
import hashlib
import json
import os
import random

from helpers import GOLD, assemble

import blocks_cases

RANGES = [(0, 4999), (5000, 9999), (10000, 13999), (14000, 17999), (18000, 21999)]      # two reference sequences, three contigs; (begin, '$')
SEP = 9999                                                                                # the '$' of the last reference sequence: rlength
NREF = 2
FUNCTION = dict(rearrangecost=1000, inversioncost=1, lastn=50, lastbp=10000, _lambda=5, eps=1, alfa=1, gapopen=10)          # glocalchain's own defaults
COMMAND = dict(rearrangecost=10000, inversioncost=5, lastn=50, lastbp=20000, _lambda=3, eps=2, alfa=2, gapopen=1)           # `reveal transform`'s
SMALL = dict(rearrangecost=60, inversioncost=3, lastn=50, lastbp=10000, _lambda=2, eps=1, alfa=1, gapopen=4)                 # the scale of the small lists below
LONG = 200      # chains above this length are kept as count + digest


def rand_blocks(rng, n, ranges=RANGES, nref=NREF, noise=0.35, maxlen=120):
    """n distinct blocks: most of them along a few (anti-)diagonals between a reference sequence and a contig, the rest anywhere"""
    out, seen = [], set()
    lines = []
    for _ in range(5):
        r, c, o = rng.randrange(nref), rng.randrange(nref, len(ranges)), rng.randrange(2)
        lines.append((r, c, o, rng.randrange(-800, 800)))
    while len(out) < n:
        L = rng.randint(5, maxlen)
        if rng.random() < noise:
            r, c, o = rng.randrange(nref), rng.randrange(nref, len(ranges)), rng.randrange(2)
            a = rng.randrange(ranges[r][0], ranges[r][1] - L)
            b = rng.randrange(ranges[c][0], ranges[c][1] - L)
        else:
            r, c, o, off = rng.choice(lines)
            x = rng.randrange(0, ranges[r][1] - ranges[r][0] - L)
            a = ranges[r][0] + x
            y = x + off + rng.randrange(-3, 4) if o == 0 else (ranges[c][1] - ranges[c][0]) - x - L + off
            b = ranges[c][0] + y
            if b < ranges[c][0] or b + L > ranges[c][1]:
                continue
        blk = (a, a + L, b, b + L, o, rng.randint(1, L), r, c)
        if blk in seen:
            continue
        seen.add(blk)
        out.append(blk)
    return out


def _case(blocks, ranges=RANGES, sep=SEP, **kw):
    assert len(set(blocks)) == len(blocks)
    return dict(blocks=list(blocks), ctg2range=list(ranges), rlength=sep, qlength=ranges[-1][1] + 1 - sep, kw=dict(SMALL, **kw))


# seeds of the multi-pass lists: tools/gen_glocal_golden.py asserts the property behind each name on the reference's own loops
PASS_SEEDS = {"passes_second_drops": (3, 90, 3), "passes_four": (6, 130, 2)}      # name -> (seed, blocks, lastn)


def cases():
    """name -> dict(blocks, ctg2range, rlength, qlength, kw): kw as glocalchain_python takes it (without axis)"""
    C = {}
    C["empty"] = _case([])
    C["one"] = _case([(100, 180, 10100, 10180, 0, 80, 0, 2)])
    C["one_rc"] = _case([(5100, 5180, 14100, 14180, 1, 80, 1, 3)])
    # two blocks share s1, two share s2: the first filter on either axis; scores differ so the sort's second component decides
    C["equal_c1"] = _case([(100, 150, 10100, 10150, 0, 50, 0, 2), (100, 190, 10300, 10390, 0, 90, 0, 2), (300, 360, 10300, 10360, 0, 60, 0, 2),
                           (500, 540, 10500, 10540, 0, 40, 0, 2)])
    # a predecessor that ends at or behind the block's end (on either axis)
    C["pred_end_ge"] = _case([(100, 900, 10100, 10900, 0, 700, 0, 2), (200, 300, 10950, 11050, 0, 100, 0, 2), (400, 900, 11100, 11600, 0, 90, 0, 2),
                              (950, 1000, 10200, 10250, 0, 50, 0, 2), (1100, 1200, 11700, 11800, 0, 100, 0, 2)])
    # a predecessor contained in the block on the other axis
    C["contained_other_axis"] = _case([(100, 200, 10500, 10600, 0, 100, 0, 2), (300, 900, 10400, 11000, 0, 500, 0, 2), (1000, 1100, 11100, 11200, 0, 100, 0, 2),
                                       (250, 280, 10650, 10680, 0, 30, 0, 2)])
    # o = 1 blocks next to the sequence ends: the dummy made relative to a block of either orientation
    C["rc_next_to_dummies"] = _case([(10, 90, 13900, 13980, 1, 80, 0, 2), (4900, 4990, 10010, 10100, 1, 90, 0, 2), (2000, 2100, 12000, 12100, 1, 100, 0, 2),
                                     (5010, 5100, 17900, 17990, 1, 90, 1, 3), (9900, 9990, 14010, 14100, 1, 90, 1, 3), (7000, 7100, 16000, 16100, 0, 100, 1, 3),
                                     (20, 80, 18020, 18080, 0, 60, 0, 4)])
    # same reference sequence / other contig, same contig / other reference sequence, both different, and mixed orientations inside one pair
    C["cross"] = _case([(100, 200, 10100, 10200, 0, 100, 0, 2), (300, 400, 14100, 14200, 0, 100, 0, 3), (500, 600, 14300, 14400, 1, 100, 0, 3),
                        (5100, 5200, 14500, 14600, 0, 100, 1, 3), (5300, 5400, 18100, 18200, 1, 100, 1, 4), (700, 800, 10300, 10400, 1, 100, 0, 2),
                        (900, 1000, 10500, 10600, 0, 100, 0, 2), (5500, 5600, 10700, 10800, 0, 100, 1, 2)], eps=0, rearrangecost=30)
    C["cross_eps"] = _case(C["cross"]["blocks"], rearrangecost=5000)
    # one long block over twenty small ones: `deepest` holds the window open beyond lastn and lastbp
    span = [(100, 3000, 10100, 13000, 0, 300, 0, 2)] + [(200 + 130 * k, 260 + 130 * k, 10230 + 130 * k, 10290 + 130 * k, 0, 55, 0, 2) for k in range(20)]
    span += [(3100, 3200, 13100, 13200, 0, 100, 0, 2), (3300, 3400, 13300, 13400, 0, 100, 0, 2)]
    C["long_span"] = _case(span, lastn=2, lastbp=10)
    C["long_span_rc"] = _case([(a, b, 24000 - d, 24000 - c, 1, s, r, g) for a, b, c, d, _, s, r, g in span], lastn=2, lastbp=10)
    # windows cut short
    base70 = rand_blocks(random.Random(70), 70)
    for lastn in (1, 2, 3, 8):
        for lastbp in (0, 10, 100):
            C["window_n%d_bp%d" % (lastn, lastbp)] = _case(base70, lastn=lastn, lastbp=lastbp)
    # windows of more than 64 edges: a step takes a second round of lanes (and, with a low edge budget, the list takes several tiles)
    C["lastn100_150"] = _case(rand_blocks(random.Random(150), 150), lastn=100)
    # the k-th of these blocks looks back over exactly k entries (lastn above the list length): 64 edges and 65 edges are among them
    C["edges_64_65"] = _case([(20 + 70 * k, 60 + 70 * k, 10020 + 50 * k, 10060 + 50 * k, 0, 30 + k % 7, 0, 2) for k in range(66)], lastn=1000, lastbp=10 ** 6)
    # ties at nearly every step: the nearest predecessor wins
    C["ties"] = _case(rand_blocks(random.Random(71), 70), rearrangecost=0, inversioncost=0, _lambda=0, eps=0, gapopen=0, alfa=1)
    C["ties_alfa0"] = _case(rand_blocks(random.Random(72), 70), rearrangecost=0, inversioncost=0, _lambda=0, eps=0, gapopen=0, alfa=0)
    C["defaults_function"] = _case(rand_blocks(random.Random(73), 120), **FUNCTION)
    C["defaults_command"] = _case(rand_blocks(random.Random(74), 120), **COMMAND)
    # 64-bit: coordinates above 2^40, weights 1024, scores that need the two-pass sort beside the positions
    base = 1 << 40
    wr = [(0, base + 4999)] + [(base + s, base + e) for s, e in RANGES[1:]]      # the first reference sequence is 2^40 long, its blocks lie in its tail
    for o in (0, 1):
        rng = random.Random(80 + o)
        wb = []
        for s1, e1, s2, e2, oo, sc, r, c in rand_blocks(rng, 60, [(base, base + 4999)] + wr[1:]):
            wb.append((s1, e1, s2, e2, oo if o else 0, sc << 20, r, c))
        C["wide_o%d" % o] = _case(wb, wr, base + SEP, rearrangecost=1024 * 60, inversioncost=1024, _lambda=1024, eps=1024, alfa=1024, gapopen=1024)
    # several passes
    for name, (seed, n, lastn) in PASS_SEEDS.items():
        C[name] = _case(rand_blocks(random.Random(seed), n), lastn=lastn, lastbp=20)
    # what the library's integer arithmetic refuses: the Python route
    C["refuse_fraction"] = _case(rand_blocks(random.Random(90), 40), _lambda=0.5, eps=0.25)
    C["refuse_huge"] = _case(rand_blocks(random.Random(91), 40), alfa=1 << 58, rearrangecost=1 << 59)
    return C


REFUSED = ("refuse_fraction", "refuse_huge")
FILTERED = ("empty", "one", "cross", "long_span", "window_n2_bp10", "window_n3_bp0", "lastn100_150", "ties", "defaults_command", "wide_o0", "wide_o1",
            "passes_second_drops", "passes_four", "refuse_fraction", "refuse_huge")      # the cases that also run both loops


def multi_blocks():
    """the block list of blocks_cases.multi_case() as the golden file of getblocks holds it (forward, then reverse complement) + its ranges"""
    T, nsep, nodes = assemble(blocks_cases.multi_inputs())
    g = blocks_cases.golden()["multi"]
    blocks = [tuple(b) for b in g["rc0"]["blocks"] + g["rc1"]["blocks"]]
    return blocks, nodes, nsep[0], len(T) - nsep[0]


def digest(idx):
    return hashlib.sha256(json.dumps([int(i) for i in idx]).encode()).hexdigest()


def golden():
    with open(os.path.join(GOLD, "glocal.json")) as f:
        return json.load(f)


def chain_record(idx):
    idx = [int(i) for i in idx]
    return dict(count=len(idx), sha256=digest(idx)) if len(idx) > LONG else idx


def indices(blocks, chain):
    """the input indices of a chain of blocks (no two blocks of a list are equal)"""
    pos = {tuple(b): i for i, b in enumerate(blocks)}
    return [pos[tuple(b)] for b in chain]


def matches(idx, rec):
    if isinstance(rec, dict):
        return len(idx) == rec["count"] and digest(idx) == rec["sha256"]
    return [int(i) for i in idx] == rec
