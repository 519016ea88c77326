"""CPU suite: the host side of the chaining programme in device memory (csrc/rv_kchain_big.hip) -- the cases of tests/golden/kchain_big.json rebuild to
the reference's results through `rv_kchain` (whose preparation both legs share), and the preparation refuses, one by one, what the device does not take."""
import json
import os

import pytest

import kchain_big_cases as B
import kchain_cases as C
from helpers import GOLD
from reveal_amd import kchain as K

with open(os.path.join(GOLD, "kchain_big.json")) as f:
    BIG = json.load(f)

R = K.KCHAIN_REFUSE


def test_constants():
    assert B.T == K.KCHAIN_BIG_TILE and K.KCHAIN_BIG_CAP == 1 << 20 and 1 <= K.KCHAIN_BIG_MIN <= K.KCHAIN_CAP + 1


def test_the_cases_cover_the_tiles():
    T = B.T
    cases = BIG["cases"]
    for k in (2, 3):
        assert {c["m"] for c in cases if c["tag"] == "random" and c["k"] == k} == {0, 1, 2, T - 1, T, T + 1, 2 * T, 3 * T + 5}
    assert {c["m"] for c in cases if c["tag"] == "random" and c["k"] == 8} == {T + 1, 2 * T + 3}
    assert {c["m"] for c in cases if c["tag"] == "random" and c["k"] == 64} == {T + 1}
    rnd = [c for c in cases if c["tag"] == "random"]
    assert {c["gcmodel"] for c in rnd} == set(B.MODELS) and {(c["wpen"], c["wscore"]) for c in rnd} == {(1, 1), (3, 1), (1, 4)} and {c["noise"] for c in rnd} == {0.1, 0.4}
    for place in B.TIE_PLACEMENTS:
        assert sum(1 for c in cases if c["tag"] == "tie_" + place) >= 2
    assert [c["k"] for c in cases if c["tag"] == "p1_stays"] == [2, 3]
    cap = [c for c in cases if c["tag"] == "cap_equal"]
    assert len(cap) == 1 and cap[0]["m"] == 2 * T + 9 and cap[0]["maxmums"] == T + 1 and cap[0]["kept"] == T + 1
    assert [c["m"] for c in cases if c["tag"] == "wide"] == [T + 5] and [c["kept"] for c in cases if c["tag"] == "above_cap"] == [1300]
    assert BIG["recurse"]["top"] > K.KCHAIN_CAP


@pytest.mark.parametrize("case", BIG["cases"], ids=lambda c: "%s-k%d-%s" % (c["tag"], c["k"], c.get("m", c["seed"])))
def test_cases_rebuild_to_the_golden_digests(case):
    recs, lens = B.build(case)
    assert B.n_kept(case) == case["kept"]
    p = B.params(case)
    path, end = K.kchain_native(recs, lens, p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"])
    assert C.digest(path, end) == case["digest"] and len(path) == case["nodes"]
    if case["kept"]:
        assert K.kchain_admit(recs, lens, p["maxmums"], p["wpen"], p["wscore"]) == 0


def test_tie_cases_are_decided_by_the_kd_order():
    for case in BIG["cases"]:
        if case["kind"] == "tie":
            recs, lens = B.build(case)
            assert K.kchain_python(recs, lens)[0] != K.kchain_python(recs, lens, tie="dim0")[0]
            pts = sorted(tuple(sorted(q for _, q in mem)) for _, _, mem in recs)
            x, y = pts[case["front"]], pts[case["front"] + 1]      # the mirrored pair, where the placement puts it
            assert x[0] < y[0] and x[-1] - (sum(lens[:-1]) + len(lens) - 1) == y[0] and len({r[0] for r in recs if tuple(sorted(q for _, q in r[2])) in (x, y)}) == 1


def rec(l, *pos):
    return (l, len(pos), tuple(enumerate(pos)))


def test_the_preparation_refuses_what_the_device_does_not_take():
    lens = [50, 50]
    ok = [rec(3, 5, 51 + 6), rec(4, 10, 51 + 20)]
    assert K.kchain_admit(ok, lens) == 0
    assert K.kchain_admit([], lens) == 0
    # a record of length 0
    l0 = [rec(0, 5, 51 + 6), rec(4, 10, 51 + 20)]
    assert K.kchain_admit(l0, lens) == R["l0"]
    # a coordinate shared by two points (dimension 0), also with p2 (dimension 1: a match that ends where the sequence does not begin)
    shared = [rec(3, 5, 51 + 6), rec(4, 5, 51 + 20)]
    assert K.kchain_admit(shared, lens) == R["shared"]
    # more than 64 sequences
    wide = [rec(3, *[51 * d + 7 for d in range(65)])]
    assert K.kchain_admit(wide, [50] * 65) == R["k"]
    # a length of 2^31; a point outside its sequence
    assert K.kchain_admit([rec(3, 5, (1 << 31) + 1 + 6)], [1 << 31, 50]) == R["bits"]
    assert K.kchain_admit([rec(3, 5, (1 << 31) + 6)], [(1 << 31) - 1, 50]) == 0
    assert K.kchain_admit([rec(30, 5, 51 + 30)], lens) == R["bits"]
    # the score bound: 2^20 x 2016 pairs x 64 sequences of 2^31 - 1 bases
    n = (1 << 31) - 1
    far = [rec(3, *[(n + 1) * d + 7 for d in range(64)])]
    assert K.kchain_admit(far, [n] * 64, 0, 1 << 20, 1) == R["score"]
    assert K.kchain_admit(far, [n] * 64, 0, 1, 1 << 20) == R["score"]      # (the gains: 2^20 x 2016 x 2^31 is 2^62 already)
    assert K.kchain_admit(far, [n] * 64, 0, 1, 1 << 10) == 0
    assert K.kchain_admit(far, [n] * 64, 0, 1, 1) == 0
    # the cap counts the kept points
    assert K.kchain_admit(l0, lens, maxmums=1) == 0
    # rv_kchain's results do not change with any of it
    for recs, ln in ((l0, lens), (shared, lens), (ok, lens), ([rec(30, 5, 51 + 30)], lens), (wide, [50] * 65)):
        assert K.kchain_native(recs, ln) == K.kchain_python(recs, ln)
    path, end = K.kchain_native(far, [n] * 64, 0, 1 << 10, 1)
    assert len(path) == 1 and end == K.kchain_python(far, [n] * 64, 0, 1 << 10, 1)[1]
