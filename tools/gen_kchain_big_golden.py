#!/usr/bin/env python3
"""Golden file of the tests of the chaining programme in device memory (csrc/rv_kchain_big.hip) from the reference's own chain() -- TEST INFRASTRUCTURE,
build container only; runs on the CPU.  The machinery is tools/gen_kchain_golden.py's (the reference's chain(), kdtree, range_search and gapcost
converted in memory and executed).  Per case the file keeps the parameters from which tests/kchain_big_cases.py rebuilds the records, and the digest of
(path, end score): no paths, so the file stays small.  Every case is checked as there: `kchain_native` (and `kchain_python` up to 300 points) equal
the reference.  The anchors of the reference's recursion on the pair of `recurse_big_input` go in whole.

    python tools/gen_kchain_big_golden.py      # rewrites tests/golden/kchain_big.json
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gen_kchain_golden import load, random_case, reference_chain, reference_recurse, tie_case, to_records      # noqa: E402
import kchain_big_cases as B                  # noqa: E402
import kchain_cases as C                      # noqa: E402
from reveal_amd import kchain as K            # noqa: E402

T = B.T
WEIGHTS = ((1, 1), (3, 1), (1, 4))


def cases():
    out = []
    x = [0]

    def rotate():
        i = x[0]
        x[0] += 1
        return dict(gcmodel=B.MODELS[i % 3], wpen=WEIGHTS[(i // 3) % 3][0], wscore=WEIGHTS[(i // 3) % 3][1])

    def rnd(tag, k, m, noise, seed, **kw):
        c = dict(tag=tag, kind="random", k=k, m=m, span=40 * m + 200, noise=noise, seed=seed, maxmums=0, extra=3 if m else 0)
        c.update(rotate())
        c.update(kw)
        out.append(c)

    seed = 1000
    for k, ms in ((2, (0, 1, 2, T - 1, T, T + 1, 2 * T, 3 * T + 5)), (3, (0, 1, 2, T - 1, T, T + 1, 2 * T, 3 * T + 5)), (8, (T + 1, 2 * T + 3)), (64, (T + 1,))):
        for i, m in enumerate(ms):
            seed += 1
            rnd("random", k, m, (0.1, 0.4)[i % 2], seed)
    # the cap cuts through a run of equal lengths
    rnd("cap_equal", 2, 2 * T + 9, 0.1, 2001, equal_l=17, maxmums=T + 1, span=20000, extra=0)
    # weights of 65536, half of the sequences running on 200 000 bases: the end score passes 2^32
    rnd("wide", 2, T + 5, 0.3, 2002, span=100000, run_on=200000, wpen=65536, wscore=65536, gcmodel="sumofpairs", extra=0)
    # above the cap of the rounds' kernel
    rnd("above_cap", 2, 1300, 0.1, 2003, extra=0)
    # the kd-order tie rule decides, across a tile boundary: kept where deciding the same ties by dimension 0 gives another path
    for place, front in B.TIE_PLACEMENTS.items():
        kept = 0
        for s in range(400):
            c = dict(tag="tie_" + place, kind="tie", k=(2, 2, 3)[s % 3], front=front, seed=3000 + s, maxmums=0, wpen=1, wscore=1, gcmodel="sumofpairs")
            recs, lens = B.build(c)
            if K.kchain_python(recs, lens)[0] != K.kchain_python(recs, lens, tie="dim0")[0]:
                out.append(c)
                kept += 1
                if kept == 2:
                    break
        assert kept == 2, (place, kept)
    out.append(dict(tag="p1_stays", kind="p1_stays", k=2, seed=4001, maxmums=0, wpen=1, wscore=1, gcmodel="sumofpairs"))
    out.append(dict(tag="p1_stays", kind="p1_stays", k=3, seed=4002, maxmums=0, wpen=3, wscore=1, gcmodel="sumofpairs"))
    return out


def check_builders():
    """tests/kchain_big_cases.py restates random_case / to_records; tie_points is tie_case with the number of points in front given"""
    for seed in range(20):
        k, m = (2, 3, 8)[seed % 3], 5 + 7 * seed
        a = random_case(random.Random(seed), k, m, 40 * m + 200, 0.3, equal_l=17 if seed % 2 else None)
        b = B.random_case(random.Random(seed), k, m, 40 * m + 200, 0.3, equal_l=17 if seed % 2 else None)
        assert a == b
        assert to_records(random.Random(seed), a[0], a[1], a[2], 3) == B.to_records(random.Random(seed), b[0], b[1], b[2], 3)
    for seed in range(200):      # tie_case draws the number of points in front itself: with that number given, the shapes are the same
        r1 = random.Random(seed)
        r1.randint(20, 40); r1.randint(45, 70); r1.randint(5, 20)
        front = r1.randint(0, 3)
        assert tie_case(random.Random(seed), 2 + seed % 2) == B.tie_points(FrontRng(seed, front), 2 + seed % 2, front)


class FrontRng:
    """a generator that skips the draw tie_case spends on the number of points in front"""

    def __init__(self, seed, front):
        self._r, self._n, self._front = random.Random(seed), 0, front
        self.shuffle = self._r.shuffle

    def randint(self, a, b):
        self._n += 1
        if self._n == 4:
            assert self._r.randint(0, 3) == self._front
        return self._r.randint(a, b)


def main():
    chain = load()
    check_builders()
    gold = []
    for c in cases():
        recs, lens = B.build(c)
        assert (recs, lens) == B.build(c, dict(to_records=to_records, random_case=random_case))
        p = B.params(c)
        path, end = reference_chain(chain, recs, lens, p)
        native = K.kchain_native(recs, lens, p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"])
        assert native == (path, end), (c, native[1], end)
        if B.n_kept(c) <= 300:
            assert K.kchain_python(recs, lens, p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"]) == (path, end), c
        if c["tag"] == "cap_equal":
            srt = sorted(r[0] for r in recs)
            assert srt[len(srt) - c["maxmums"] - 1] == srt[len(srt) - c["maxmums"]]
        if c["tag"] == "wide":
            assert abs(end) > 1 << 32
        if c["tag"] == "p1_stays":      # the node keeps p1: its score is p1's offer
            node = (200, 110) if c["k"] == 2 else (200, 110, 205)
            begin = [sum(lens[:d]) + d for d in range(c["k"])]
            pts = sorted(tuple(q - begin[d] for d, q in enumerate(sorted(q for _, q in mem))) for _, _, mem in recs)
            assert pts.index(node) >= T and all(v[1] > node[1] for v in pts[1:pts.index(node)])
            if node in [v for _, v, _ in path]:
                assert [sc for _, v, sc in path if v == node] == [-p["wpen"] * K.gapcost(tuple([-1] * c["k"]), node, p["gcmodel"])]
        if c["kind"] != "random" or c["m"] > 0:
            assert K.kchain_admit(recs, lens, p["maxmums"], p["wpen"], p["wscore"]) == 0, c
        gold.append(dict(c, digest=C.digest(path, end), nodes=len(path), kept=B.n_kept(c)))
        print(c["tag"], c["k"], c.get("m", c.get("front")), len(path), end)
    seqs = list(B.recurse_big_input())
    top = sum(1 for r in C.oracle_records(tuple(seqs), C.RECURSE_PARAMS["minlength"]) if r[1] == 2)
    assert top > 1024, top
    anchors, maxdepth = reference_recurse(chain, seqs, C.RECURSE_PARAMS)
    gen = "tools/gen_kchain_big_golden.py: reveal/chain.py chain + reveal/utils.py kdtree / range_search / gapcost, converted in memory (lib2to3) and executed"
    with open(os.path.join(ROOT, "tests", "golden", "kchain_big.json"), "w") as f:
        json.dump({"_generator": gen, "cases": gold, "recurse": dict(top=top, maxdepth=maxdepth, anchors=[[l, [list(x) for x in mem], d] for l, mem, d in anchors])},
                  f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("wrote kchain_big.json", len(gold), "cases;", top, "full matches at the top level,", len(anchors), "anchors, depth", maxdepth)


if __name__ == "__main__":
    main()
