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


# ---- the large cases: what the kernels of rv_glocal.hip do above one workgroup, above 192 edges a window and above the 2048 scores of the LDS ring.
# Their records stand under "large" in the golden file; reach() states, per case and axis, the arithmetic that takes it to the line it is there for
# (tests/test_cpu_glocal.py::test_large_reach asserts it on the CPU, the GPU tests assert the counts the library reports).
WG = 256                 # threads of a per-entry kernel: gm = ceil((m + 2) / WG) workgroups
SCAN_TILE = 2048         # items of a scan tile (rv_prims.hip)
RING = 2048              # GLC_RING: the scores k_glc_chain keeps in LDS
AHEAD = 192              # GLC_NR * 64: the edges of a window that k_glc_chain loads ahead; the rest is its tail loop
NDUMMY = (2, 3)          # dummies per axis with RANGES and with LONG_RANGES: two reference sequences, three contigs
LONG_RANGES = [(0, 49999), (50000, 54999), (55000, 104999), (105000, 108999), (109000, 112999)]      # room for a thousand blocks on one diagonal
LONG_SEP = 54999
RING_TILE_BUDGET = 500000                                # ring_2300 under this edge budget: six tiles, the last one begins behind entry RING
PASSES_BIG = (1, 2300, 2)                                # (seed, blocks, lastn): tools/gen_glocal_golden.py asserts three passes and > WG survivors
FAR = ((191, 0), (191, 1), (192, 0), (192, 1), (2047, 0), (2048, 0))      # (entries between a block and its best predecessor, the axis it is built on)
COLLINEAR = (253, 254, 1021, 1022)


def collinear_blocks(n):
    """n blocks that do not overlap, on one diagonal of the first reference sequence and the first contig"""
    rng = random.Random(n)
    out = []
    for k in range(n):
        L = rng.randint(8, 30)
        out.append((10 + 40 * k, 10 + 40 * k + L, 55010 + 40 * k, 55010 + 40 * k + L, 0, rng.randint(1, L), 0, 2))
    return out


def far_blocks(between, axis):
    """A block B whose best predecessor lies `between` entries back in the sorted order of `axis`: 40 blocks A on a diagonal, then `between` blocks
    whose other coordinate lies below every A and falls from one to the next (o = 0: reaching one of them, or leaving one for a block further up,
    is a rearrangement), then B and ten more on the diagonal of A.  With eps = 0 the step A[39] -> B costs gapopen alone.  -> (blocks, index of
    A[39], index of B)"""
    lay = [(2 + 20 * i, 10, 30002 + 20 * i, 8 + i % 3) for i in range(40)]                      # (begin on the axis, length, begin on the other, score)
    lay += [(1000 + 8 * t, 4, 25000 - 10 * t, 1 + t % 3) for t in range(between)]
    p0 = 1000 + 8 * between + 20
    lay += [(p0 + 20 * i, 10, 30000 + p0 + 20 * i, 9 + i % 2) for i in range(11)]
    out = []
    for p, L, s, sc in lay:
        out.append((p, p + L, 55000 + s, 55000 + s + L, 0, sc, 0, 2) if axis == 0 else (s, s + L, 55000 + p, 55000 + p + L, 0, sc, 0, 2))
    return out, 39, 40 + between


def large_cases():
    """name -> case, as cases(): the smallest lists that reach the lines named beside them"""
    C = {}
    # m + 2 = 254 .. 258 over the two axes: the second workgroup of every per-entry kernel and their guards k > m, k <= m + 1
    for n in (250, 251, 252, 253):
        C["entries_256_%d" % n] = _case(rand_blocks(random.Random(n), n))
    # the longest path a list can have, m + 1 on axis 0 = 256, 257, 1024, 1025: every launch of k_glc_double is needed at a power of two
    for n in COLLINEAR:
        C["collinear_%d" % n] = _case(collinear_blocks(n), LONG_RANGES, LONG_SEP, _lambda=2, eps=0, gapopen=0, rearrangecost=60, alfa=1)
    # the k-th entry looks back over exactly k entries: windows of 191, 192, 193, 256, 257 edges -- the tail loop of k_glc_chain behind AHEAD edges
    # (every fifth block lies 20 off the line the others follow, and a block gains 16 .. 26 against 15 for a step along it: 206 of them are kept)
    off = [20 if k % 5 == 2 else 0 for k in range(260)]
    C["window_260"] = _case([(20 + 19 * k, 32 + 19 * k, 10020 + 15 * k + off[k], 10032 + 15 * k + off[k], 0, 16 + 7 * k % 11, 0, 2) for k in range(260)],
                            lastn=1000, lastbp=10 ** 6)
    # the same with 2300 random blocks: windows above RING edges (scores read from global memory), three scans over two scan tiles, ten workgroups;
    # under RING_TILE_BUDGET a tile that begins behind entry RING (the ring's pre-load from klo - RING > 0)
    C["ring_2300"] = _case(rand_blocks(random.Random(2300), 2300), lastn=3000, lastbp=10 ** 6)
    # the best predecessor at a known distance: the last edge loaded ahead and the first of the tail loop, the last score in the ring and the first
    # outside it
    for between, axis in FAR:
        C["far_%d_axis%d" % (between, axis)] = _case(far_blocks(between, axis)[0], LONG_RANGES, LONG_SEP, lastn=3000, lastbp=10 ** 6, rearrangecost=100,
                                                      inversioncost=0, _lambda=5, eps=0, alfa=1, gapopen=1)
    # several passes over a list of ten workgroups: compaction into a second pass of more than WG entries
    seed, n, lastn = PASSES_BIG
    C["passes_big"] = _case(rand_blocks(random.Random(seed), n), lastn=lastn, lastbp=20)
    # the two-sort route (coordinates above 2^40) above one workgroup: the second sort's permutation gathered by three
    base = 1 << 40
    wr = [(0, base + 4999)] + [(base + s, base + e) for s, e in RANGES[1:]]
    for o in (0, 1):
        rng = random.Random(600 + o)
        wb = [(s1, e1, s2, e2, oo if o else 0, sc << 20, r, c) for s1, e1, s2, e2, oo, sc, r, c in rand_blocks(rng, 600, [(base, base + 4999)] + wr[1:])]
        C["wide_600_o%d" % o] = _case(wb, wr, base + SEP, rearrangecost=1024 * 60, inversioncost=1024, _lambda=1024, eps=1024, alfa=1024, gapopen=1024)
    return C


LARGE_FILTERED = ("entries_256_250", "entries_256_251", "entries_256_252", "entries_256_253", "passes_big", "wide_600_o0", "wide_600_o1")
WHOLE_PREFIX = ("window_260", "ring_2300") + tuple("far_%d_axis%d" % f for f in FAR)      # the window of the k-th entry is the k entries in front of it
LARGE_BUDGETS = {"window_260": (64, 1000), "ring_2300": (RING_TILE_BUDGET,)}              # the cases that also run under a low edge budget


def entries(c, axis):
    """m of a pass over the whole list: the blocks and the dummies of the axis"""
    nd = sum(1 for s, _ in c["ctg2range"] if (s < c["rlength"]) == (axis == 0))
    return len(c["blocks"]) + nd


def whole_prefix_edges(m):
    return m * (m + 1) // 2


def doubling_launches(m):
    """launches of k_glc_double: ceil(log2(m + 1)); after t of them the marks reach 2^t - 1 steps down the path from `end`"""
    return (m).bit_length()


def first_entry_of_tile(tile, budget):
    """whole-prefix windows, eoff[k] = k (k - 1) / 2: the first entry whose first edge lies at or behind tile * budget"""
    k = 1
    while k * (k - 1) // 2 < tile * budget:
        k += 1
    return k


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
