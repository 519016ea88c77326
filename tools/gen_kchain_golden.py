#!/usr/bin/env python3
"""Golden files of the kchain tests from the reference's own chain() (reveal/chain.py:214-314) -- TEST INFRASTRUCTURE, build container only.

The reference is Python 2.  This script converts reveal/chain.py and reveal/utils.py IN MEMORY with lib2to3 (nothing of them is written to the
repository), pulls `chain`, `kdtree`, `range_search` and `gapcost` out of the converted syntax trees and executes THEM, with Python 2's floor
division restored and networkx 1's `.node[` spelled `.nodes[`.  chain() runs on a stand-in index object (nsamples, nsep, n, getmultimums, getmums)
whose lists are given (the abstract cases) or come from the CPU oracle on the job alone (tests/kchain_cases.py oracle_records).  A job of two
sequences is handed to chain() in the multi-MUM shape (l, 2, ((0, a), (1, b))): with the shape getmums ships, chain()'s own filter drops every
record (reveal_amd/kchain.py, "the one deliberate departure").  A job without a full match has no scored end sentinel in the reference; the files
hold -wpen gapcost(p1, p2) for it, what the programme would give.

    python tools/gen_kchain_golden.py      # rewrites tests/golden/kchain_vectors.json, many_kchain.json, kchain_recurse.json
"""
import ast
import json
import logging
import math
import os
import random
import sys
from lib2to3 import refactor

import networkx as nx

REF = "/root/reference/reveal"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kchain_cases as C                      # noqa: E402
from reveal_amd import kchain as K            # noqa: E402


def convert(path):
    tool = refactor.RefactoringTool(refactor.get_fixers_from_package("lib2to3.fixes"))
    src = open(path).read()
    if not src.endswith("\n"):
        src += "\n"
    return str(tool.refactor_string(src, path)).replace(".node[", ".nodes[")


class FloorDiv(ast.NodeTransformer):
    def visit_BinOp(self, node):
        self.generic_visit(node)
        if isinstance(node.op, ast.Div):
            node.op = ast.FloorDiv()
        return node


def functions(path, names):
    tree = ast.parse(convert(path))
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == set(names), (path, names)
    return compile(ast.fix_missing_locations(FloorDiv().visit(ast.Module(body=body, type_ignores=[]))), path, "exec")


def load():
    env = {"logging": logging, "log": math.log, "nx": nx}
    exec(functions(os.path.join(REF, "utils.py"), {"gapcost", "kdtree", "range_search"}), env)
    exec(functions(os.path.join(REF, "chain.py"), {"chain"}), env)
    return env["chain"]


class Index:
    """what chain() reads of an index: the list in the multi-MUM shape for every k"""

    def __init__(self, records, lens):
        self.nsamples = len(lens)
        self.n = sum(lens) + len(lens)
        self.nsep = [sum(lens[:d + 1]) + d for d in range(len(lens) - 1)]
        self._records = [(l, n, tuple(tuple(x) for x in mem)) for l, n, mem in records]

    def getmultimums(self, minlength=0, minn=2):
        return list(self._records)

    def getmums(self, minlength=0):
        return list(self._records)


def reference_chain(chain, records, lens, p):
    """-> (path [(l, point, score)], end_score) of the reference's chain() with offsets all zero"""
    k = len(lens)
    begin = [sum(lens[:d]) + d for d in range(k)]
    full = [tuple(sorted(q for _, q in mem)) for _, n, mem in records if n == k]
    for d in range(k):      # two full multi-MUMs cannot start at the same position of a sequence: kdtree's `splitvalue += 1` is never taken
        col = [pt[d] - begin[d] for pt in full] + [lens[d]]
        assert len(set(col)) == len(col), "a coordinate shared by two points in dimension %d" % d
    G, p1, p2, path = chain(Index(records, lens), tuple([0] * k), p.get("minlength", 20), 0, p["maxmums"], gcmodel=p["gcmodel"], wpen=p["wpen"], wscore=p["wscore"])
    assert path[0] == p1 and path[-1] == p2
    if len(path) == 2 and "score" not in G.nodes.get(p2, {}):
        return [], -p["wpen"] * K.gapcost(p1, p2, p["gcmodel"])
    return [(G.nodes[v]["l"], tuple(v), G.nodes[v]["score"]) for v in path[1:-1]], G.nodes[p2]["score"]


# ---- abstract cases ----
def to_records(rng, pts, ls, lens, extra=0):
    """points (relative) -> records in the coordinates of the job's text, members shuffled; `extra` records of fewer sequences among them"""
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
    cols = [sorted(rng.sample(range(span), m)) for _ in range(k)]      # distinct coordinates in every dimension
    pts = [[cols[d][i] for d in range(k)] for i in range(m)]
    for d in range(1, k):      # a share of the points off the backbone in this dimension: swap coordinates between points
        for _ in range(int(noise * m)):
            a, b = rng.randrange(m), rng.randrange(m)
            pts[a][d], pts[b][d] = pts[b][d], pts[a][d]
    ls = [equal_l if equal_l and rng.random() < 0.7 else rng.randint(1, lmax) for _ in range(m)]
    order = list(range(m))
    rng.shuffle(order)
    lens = [span + lmax + rng.randint(0, 30) for _ in range(k)]
    return [tuple(pts[i]) for i in order], [ls[i] for i in order], lens


def tie_case(rng, k):
    """a pair of equal-length matches mirrored about the diagonal in front of a common successor, among a few collinear ones"""
    a, b = rng.randint(20, 40), rng.randint(45, 70)
    l = 2 * (b - a) + rng.randint(5, 20)      # (long enough that taking one of the two beats skipping both)
    pts, ls = [], []
    at = 0
    for _ in range(rng.randint(0, 3)):      # collinear ones in front
        at += rng.randint(15, 30)
        pts.append(tuple([at] * k)); ls.append(rng.randint(3, 10))
    o = at + 20
    x = [o + a] * k
    y = [o + b] * k
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


def abstract_vectors(chain):
    rng = random.Random(20261020)
    out = []

    def add(tag, pts, ls, lens, extra=0, **kw):
        p = dict(maxmums=0, wpen=1, wscore=1, gcmodel="sumofpairs")
        p.update(kw)
        recs = to_records(rng, pts, ls, lens, extra)
        path, end = reference_chain(chain, recs, lens, p)
        mine = K.kchain_python(recs, lens, p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"])
        assert mine == (path, end), (tag, mine, path, end)
        out.append(dict(tag=tag, k=len(lens), lens=lens, records=[[l, n] + [x for sp in mem for x in sp] for l, n, mem in recs], maxmums=p["maxmums"], wpen=p["wpen"],
                        wscore=p["wscore"], gcmodel=p["gcmodel"], path=[[l, list(v), sc] for l, v, sc in path], end_score=end))
        return recs, path, p

    models = ("sumofpairs", "star-avg", "star-med")
    x = 0
    for k in (2, 3, 8, 16, 64):
        for m in {2: (0, 1, 2, 7, 30, 200), 3: (0, 1, 7, 30), 8: (0, 1, 12), 16: (0, 3), 64: (0, 2)}[k]:      # (sized to keep the file small)
            for noise in (0.1, 0.4) if 2 <= m <= 30 and k <= 8 else (0.2,):
                pts, ls, lens = random_case(rng, k, m, 40 * m + 200, noise)
                add("random", pts, ls, lens, extra=3 if m else 0, gcmodel=models[x % 3], wpen=(1, 3, 1)[x % 3], wscore=(1, 1, 4)[(x // 3) % 3])
                x += 1
    # the kd-order tie rule decides: kept where deciding the same ties by dimension 0 gives another path
    decided = 0
    for _ in range(400):
        k = rng.choice((2, 2, 3))
        pts, ls, lens = tie_case(rng, k)
        recs = to_records(rng, pts, ls, lens)
        if K.kchain_python(recs, lens)[0] != K.kchain_python(recs, lens, tie="dim0")[0]:
            add("tie", pts, ls, lens)
            decided += 1
            if decided == 10:
                break
    assert decided >= 10, decided
    # the cap cuts through a run of equal lengths
    for i in range(6):
        k = (2, 3, 2, 3, 2, 8)[i]
        pts, ls, lens = random_case(rng, k, 16, 3000, 0.1, equal_l=17)
        srt = sorted(ls)
        cut = next(c for c in range(3, len(ls) - 3) if srt[len(ls) - c - 1] == srt[len(ls) - c])
        add("cap_equal", pts, ls, lens, maxmums=cut, gcmodel=models[i % 3])
    for mm in (1, 11, 12, 13):
        pts, ls, lens = random_case(rng, 2, 12, 3000, 0.1)
        add("cap", pts, ls, lens, maxmums=mm)
    # p1 stays the best predecessor of a node that has admissible candidates
    add("p1_stays", [(0, 100), (200, 110)], [5, 6], [400, 400])
    add("p1_stays", [(0, 100, 0), (200, 110, 205), (300, 300, 300)], [5, 6, 9], [400, 400, 400], wpen=3)
    # weights of 65536: scores beyond 2^32
    for i, k in enumerate((2, 8, 64)):
        pts, ls, lens = random_case(rng, k, (12, 6, 3)[i], 100000, 0.3)
        lens = [n + (200000 if d >= k // 2 else 0) for d, n in enumerate(lens)]      # (half of the sequences run on: the end sentinel lies far off)
        _, path, _ = add("wide", pts, ls, lens, wpen=65536, wscore=(65536, 1, 65536)[i], gcmodel=models[i])
    return out


# ---- the GPU batches ----
def batch_goldens(chain):
    return {C.run_key(name, p): [C.digest(*reference_chain(chain, C.oracle_records(tuple(seqs), p["minlength"]), [len(s) for s in seqs], p)) for seqs in jobs()]
            for name, jobs in C.BATCHES.items() for p in C.RUNS[name]}


# ---- the driver: the loop of chain_cmd (chain.py:57-124), restated around the reference's chain() ----
def reference_recurse(chain, seqs, p):
    k0 = len(seqs)
    begin = [sum(len(s) for s in seqs[:i]) + i for i in range(k0)]
    stack = [(list(range(k0)), [0] * k0, [len(s) for s in seqs], 0)]
    anchors, maxdepth = [], 0
    while stack:
        ids, offs, ends, depth = stack.pop()
        sub = [seqs[i][o:e] for i, o, e in zip(ids, offs, ends)]
        lens = [len(s) for s in sub]
        path, _ = reference_chain(chain, C.oracle_records(tuple(sub), p["minlength"]), lens, p)
        if not path:
            continue
        maxdepth = max(maxdepth, depth)
        nodes = [(l, tuple(o + q for o, q in zip(offs, pt))) for l, pt, _ in path]
        anchors += [(l, tuple((i, begin[i] + q) for i, q in zip(ids, pt)), depth) for l, pt in nodes]
        f, l = tuple(offs), 0
        for nl, pos in nodes + [(0, tuple(ends))]:
            nxt = [(ids[i], f[i] + l, pos[i]) for i in range(len(ids)) if f[i] + l < pos[i]]
            assert all(f[i] + l <= pos[i] for i in range(len(ids)))
            if len(nxt) >= p["minn"]:
                stack.append(([s[0] for s in nxt], [s[1] for s in nxt], [s[2] for s in nxt], depth + 1))
            f, l = pos, nl
    return sorted(anchors), maxdepth


def main():
    chain = load()
    gen = "tools/gen_kchain_golden.py: reveal/chain.py chain + reveal/utils.py kdtree / range_search / gapcost, converted in memory (lib2to3) and executed"

    def dump(name, key, obj):
        with open(os.path.join(ROOT, "tests", "golden", name), "w") as f:
            json.dump({"_generator": gen, key: obj}, f, sort_keys=True, separators=(",", ":"))
            f.write("\n")
        print("wrote", name, len(obj))
    dump("kchain_vectors.json", "cases", abstract_vectors(chain))
    rec = {}
    for name, seqs in C.recurse_inputs().items():
        anchors, maxdepth = reference_recurse(chain, list(seqs), C.RECURSE_PARAMS)
        rec[name] = dict(anchors=[[l, [list(x) for x in mem], d] for l, mem, d in anchors], maxdepth=maxdepth)
    dump("kchain_recurse.json", "inputs", rec)
    dump("many_kchain.json", "runs", batch_goldens(chain))


if __name__ == "__main__":
    main()
