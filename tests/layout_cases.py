"""shared cases of the layout tests (tests/test_cpu_layout.py, tests/test_gpu_layout.py) and of tools/gen_layout_golden.py, which runs the reference's
own merge_consecutive, remove_overlap_*_blocks, chainscore, optimise and extendblocks on them and writes tests/golden/layout.json.  Everything here
is seeded and deterministic; the large lists exist only as their seeds, the golden file keeps a count and a digest of what they merge into.

merge_cases(): name -> dict(blocks) or dict(rows, sel): abstract lists, nothing of them has to lie inside a sequence.
tail_cases():  name -> dict(chain, ctg2range, rlength, qlength, greedy, minchainsum, kw): lists over two reference sequences and three contigs.
"""
import hashlib
import json
import os
import random

from helpers import GOLD

RANGES = [(0, 4999), (5000, 9999), (10000, 13999), (14000, 17999), (18000, 21999)]      # two reference sequences, three contigs; (begin, '$')
SEP = 9999
NREF = 2
COMMAND = dict(rearrangecost=10000, inversioncost=5, _lambda=3, eps=2, alfa=2, gapopen=1)            # `reveal transform`'s weights
SMALL = dict(rearrangecost=60, inversioncost=3, _lambda=2, eps=1, alfa=1, gapopen=4)                  # the scale of the lists below
LONG = 64              # lists above this length are kept as count + digest
WG = 256               # threads of a workgroup of the merge kernels
HOST_BELOW = 8192      # RV_MERGE_HOST_BELOW as shipped: shorter lists take the host rule inside rv_merge_blocks
RANDOM_SEEDS = tuple(range(14))
# the tail lists: (seed, blocks, greedy, weights).  tools/gen_layout_golden.py asserts on the reference's own run that TAIL_DROPS is a case where a sweep
# drops a block, TAIL_TWO_SWEEPS one with two accepted sweeps, and that at most one case in five raises.
TAIL = tuple((seed, n, greedy, w) for seed, n in ((0, 0), (1, 1), (2, 2), (3, 7), (4, 12), (5, 20), (6, 28), (7, 36), (8, 44), (9, 52), (10, 60), (2, 33), (1, 25),
                                                  (4, 60), (1, 45))
             for greedy in (False, True) for w in ("command", "small"))
TAIL_DROPS = "tail_s2_n33_conservative_small"
TAIL_TWO_SWEEPS = "tail_s4_n60_greedy_small"


def run(first, n, o=0, ctg=2, ref=0, step=100, length=60, s1=1000, s2=1000000, score=None):
    """n collinear blocks: entries first .. first + n - 1 of a line; o = 1 walks the query backwards"""
    out = []
    for k in range(first, first + n):
        a = s1 + step * k
        b = s2 + step * k if o == 0 else s2 + step * (100000 - k)
        out.append((a, a + length, b, b + length, o, (k % 7) + 1 if score is None else score, ref, ctg))
    return out


def singles(n):
    """n blocks none of which joins its neighbour: the contig changes at every step"""
    return [(1000 + 100 * k, 1060 + 100 * k, 1000000 + 100 * k, 1000060 + 100 * k, 0, (k % 5) + 1, 0, 2 + (k & 1)) for k in range(n)]


def runs_of(rng, n, maxrun=9):
    """n entries in runs of 1 .. maxrun, orientation and contig drawn per run; the runs follow each other on both axes"""
    out, k = [], 0
    while k < n:
        L = min(rng.randint(1, maxrun), n - k)
        o, ctg = rng.randrange(2), 2 + rng.randrange(3)
        if out and out[-1][4] == o and out[-1][7] == ctg:                         # (the neighbours would join: another contig)
            ctg = 2 + (ctg - 1) % 3
        for j in range(L):
            a = 1000 + 100 * (k + j)
            b = 1000000 + 100 * (k + j) if o == 0 else 1000000 + 100 * (k + L - 1 - j)
            out.append((a, a + rng.randint(10, 90), b, b + rng.randint(10, 90), o, rng.randint(1, 500), rng.randrange(2), ctg))
        k += L
    return out


def rand_list(seed):
    """0 .. 150 blocks: pieces of a few lines, shuffled, with noise and with ties of s1 and of s2"""
    rng = random.Random(1000 + seed)
    n = [0, 1, 2, 3, 150, 149][seed] if seed < 6 else rng.randint(4, 150)
    out = []
    while len(out) < n:
        if rng.random() < 0.7:
            L = min(rng.randint(1, 12), n - len(out))
            o, ctg, ref = rng.randrange(2), 2 + rng.randrange(3), rng.randrange(2)
            a0, b0 = rng.randrange(0, 9000), rng.randrange(10000, 21000)
            for j in range(L):
                a = a0 + 40 * j
                b = b0 + 40 * j if o == 0 else b0 + 40 * (L - 1 - j)
                out.append((a, a + rng.randint(5, 39), b, b + rng.randint(5, 39), o, rng.randint(1, 300), ref, ctg))
        elif out and rng.random() < 0.5:                                         # a tie: the s1 or the s2 of a block that is there already
            t = rng.choice(out)
            a, b = (t[0], rng.randrange(10000, 21000)) if rng.random() < 0.5 else (rng.randrange(0, 9000), t[2])
            out.append((a, a + rng.randint(5, 39), b, b + rng.randint(5, 39), t[4], rng.randint(1, 300), rng.randrange(2), t[7]))
        else:
            a, b = rng.randrange(0, 9000), rng.randrange(10000, 21000)
            out.append((a, a + rng.randint(5, 39), b, b + rng.randint(5, 39), rng.randrange(2), rng.randint(1, 300), rng.randrange(2), 2 + rng.randrange(3)))
    rng.shuffle(out)
    return out


def merge_cases():
    C = {}
    A = (100, 160, 10100, 10160, 0, 60, 0, 2)
    C["empty"] = dict(blocks=[])
    C["one"] = dict(blocks=[A])
    C["join_o0"] = dict(blocks=[A, (300, 380, 10300, 10380, 0, 80, 0, 2)])
    C["join_o1"] = dict(blocks=[(100, 160, 10300, 10360, 1, 60, 0, 2), (300, 380, 10100, 10180, 1, 80, 0, 2)])
    C["o1_ranks_ascending"] = dict(blocks=[(100, 160, 10100, 10160, 1, 60, 0, 2), (300, 380, 10300, 10380, 1, 80, 0, 2)])        # o = 1 wants the rank to fall
    C["o0_ranks_descending"] = dict(blocks=[(100, 160, 10300, 10360, 0, 60, 0, 2), (300, 380, 10100, 10180, 0, 80, 0, 2)])
    C["ranks_not_adjacent"] = dict(blocks=[A, (300, 380, 10500, 10580, 0, 80, 0, 2), (5000, 5050, 10300, 10350, 0, 50, 1, 2)])     # the third lies between them in the query
    C["other_ctgid"] = dict(blocks=[A, (300, 380, 14300, 14380, 0, 80, 0, 3)])
    C["other_refid_joins"] = dict(blocks=[A, (5300, 5380, 10300, 10380, 0, 80, 1, 2)])
    C["mixed_o"] = dict(blocks=[A, (300, 380, 10300, 10380, 1, 80, 0, 2), (500, 580, 10500, 10580, 0, 70, 0, 2), (700, 780, 10700, 10780, 0, 30, 0, 2)])
    tie = [(100, 160, 10200, 10260, 0, 5, 0, 2), (100, 150, 10100, 10150, 0, 7, 1, 2), (300, 380, 10300, 10380, 0, 11, 0, 2)]
    C["equal_s1_first"] = dict(blocks=tie)                                        # R = tie[0], tie[1], tie[2]: nothing joins
    C["equal_s1_second"] = dict(blocks=[tie[1], tie[0], tie[2]])                  # R = tie[1], tie[0], tie[2]: one run
    C["equal_s2_o0"] = dict(blocks=[(100, 160, 10500, 10560, 0, 5, 0, 2), (200, 260, 10500, 10570, 0, 7, 0, 2)])      # equal s2: ranks in the order of R
    C["equal_s2_o1"] = dict(blocks=[(100, 160, 10500, 10560, 1, 5, 0, 2), (200, 260, 10500, 10570, 1, 7, 0, 2)])
    C["run_257"] = dict(blocks=run(0, 257))                                       # a single head; the run crosses a workgroup boundary
    C["run_1025_o1"] = dict(blocks=run(0, 1025, o=1))                             # ... every workgroup boundary
    C["singles_256"] = dict(blocks=singles(256))                                  # a head everywhere
    C["singles_257"] = dict(blocks=singles(257))
    S = singles(600)
    for k, b in zip(range(254, 259), run(254, 5, ctg=4)):                         # one run over entries 254 .. 258
        S[k] = b
    C["run_254_258"] = dict(blocks=S)
    C["runs_2300"] = dict(blocks=runs_of(random.Random(2300), 2300))              # more than one tile of the scans
    C["runs_2300_shuffled"] = dict(blocks=runs_of(random.Random(2301), 2300))
    random.Random(7).shuffle(C["runs_2300_shuffled"]["blocks"])
    for n in (HOST_BELOW - 1, HOST_BELOW):                                        # either side of the shipped threshold between the host rule and the kernels
        C["threshold_%d" % n] = dict(blocks=runs_of(random.Random(n), n, maxrun=40))
    W = 1 << 40
    C["wide_coordinates"] = dict(blocks=[(W + 5 * a, W + 5 * a + 3, 3 * W + 7 * b, 3 * W + 7 * b + 3, o, s, 0, c) for a, b, o, s, c in
                                         ((0, 0, 0, 9, 2), (10, 10, 0, 8, 2), (20, 20, 0, 7, 2), (30, 50, 1, 6, 2), (40, 40, 1, 5, 2), (50, 30, 1, 4, 3), (60, 25, 1, 3, 3))]
                                 + [(7, 9, 3 * W + 1000, 3 * W + 1002, 0, 1, 0, 2)])
    C["scores_2p31"] = dict(blocks=run(0, 5, score=1 << 31) + run(5, 3, ctg=3, score=1 << 31))
    rows = runs_of(random.Random(600), 600)
    sel = list(range(600))
    random.Random(601).shuffle(sel)
    sel = sel[:300]
    sel[17] = sel[3]                                                              # a row taken twice
    C["sel_600"] = dict(rows=rows, sel=sel)
    rows = runs_of(random.Random(40), 40, maxrun=20)
    C["sel_ordered"] = dict(rows=rows, sel=[k for k in range(40) if k % 7 != 3])  # rows left out of runs: their neighbours join across the hole
    for seed in RANDOM_SEEDS:
        C["random_%02d" % seed] = dict(blocks=rand_list(seed))
    return C


def merge_list(c):
    """the list a merge case stands for"""
    return list(c["blocks"]) if "blocks" in c else [c["rows"][i] for i in c["sel"]]


def tail_name(seed, n, greedy, w):
    return "tail_s%d_n%d_%s_%s" % (seed, n, "greedy" if greedy else "conservative", w)


def tail_list(seed, n):
    """n blocks of a chain as glocalchain leaves it: pieces of lines between a reference sequence and a contig whose neighbours overlap now and then,
    and a few blocks anywhere"""
    rng = random.Random(5000 + seed)
    out, seen = [], set()
    while len(out) < n:
        r, c, o = rng.randrange(NREF), rng.randrange(NREF, len(RANGES)), rng.randrange(2)
        rs, re = RANGES[r]
        cs, ce = RANGES[c]
        k = min(rng.randint(1, 9), n - len(out))
        x, off = rng.randrange(0, 2500), rng.randrange(0, 600)
        for _ in range(k):
            L = rng.randint(30, 220)
            a = rs + x
            b = cs + x + off if o == 0 else ce - (x + off) - L
            if a + L > re or b < cs or b + L > ce:
                break
            blk = (a, a + L, b, b + L, o, rng.randint(L // 2, L), r, c)
            if blk not in seen:
                seen.add(blk)
                out.append(blk)
            x += L + rng.choice((-60, -25, -8, 0, 5, 30, 90, 200))
            if rng.random() < 0.25:
                off += rng.randint(-40, 40)
    rng.shuffle(out)
    return out


def tail_cases():
    C = {}
    for seed, n, greedy, w in TAIL:
        C[tail_name(seed, n, greedy, w)] = dict(chain=tail_list(seed, n), ctg2range=list(RANGES), rlength=SEP, qlength=RANGES[-1][1] + 1 - SEP, greedy=greedy,
                                                minchainsum=50, kw=dict(COMMAND if w == "command" else SMALL))
    return C


def digest(blocks):
    return hashlib.sha256(json.dumps([[int(x) for x in b] for b in blocks], separators=(",", ":")).encode()).hexdigest()


def record(blocks):
    """what the golden file keeps of a list: the list, or for a long one its length and digest"""
    blocks = [[int(x) for x in b] for b in blocks]
    return dict(count=len(blocks), sha256=digest(blocks)) if len(blocks) > LONG else blocks


def matches(blocks, rec):
    if isinstance(rec, dict):
        return len(blocks) == rec["count"] and digest(blocks) == rec["sha256"]
    return [[int(x) for x in b] for b in blocks] == rec


def golden():
    with open(os.path.join(GOLD, "layout.json")) as f:
        return json.load(f)
