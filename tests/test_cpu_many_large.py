"""RV_MANY_LARGE without a device: the job generator of tests/test_gpu_many_large.py, the eligibility rule on both sides of 2048 ranks and
of RV_MANY_LARGE_MAX, and the coordinate mapping of the shared layout at these sizes."""
import inspect

import many_cases as mc
import many_large_cases as lc
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many


def ranks(pair):
    return len(pair[0]) + len(pair[1]) + 2


def test_generator_is_deterministic_and_in_range():
    a, b = lc.large_class_jobs(3), lc.large_class_jobs(3)
    assert a == b and len(a) == 3 * len(lc.CLASSES)
    assert lc.large_class_jobs(2, seed=5) != lc.large_class_jobs(2, seed=6)
    seen = set()
    for cls, pair in lc.large_class_jobs(12):
        assert lc.RANKS_MIN <= ranks(pair) <= lc.RANKS_MAX, (cls, ranks(pair))
        assert lc.RANKS_MIN == many.LEAF_RANKS + 1
        seen.add(cls)
    assert seen == set(lc.CLASSES)
    bare = [p for cls, p in lc.large_class_jobs(12) if cls == "homopolymer" and set(p[0]) == {"A"}]
    assert bare and all(p[1] == p[0][:-1] for p in bare)


def test_corner_sizes():
    c = lc.corner_jobs()
    assert c == lc.corner_jobs()
    assert tuple(ranks(p) for p in c) == lc.CORNER_RANKS == (2049, 2048, 3001, 4196, 4003, 20000, 20000, 80002)
    assert c[0][0] == c[1][0] and c[0][1][:1022] == c[1][1]
    assert c[2] == ("A" * 1500, "A" * 1499) and c[3] == ("ACG" * 700, "ACG" * 698) and c[4][1] == "A"
    assert c[6][0] == c[6][1] and c[5][0] != c[5][1] and c[7][0] != c[7][1]
    assert max(lc.CORNER_RANKS) > 65536


def test_generator_gives_jobs_with_anchors():
    """on the oracle alone: more than half of the large jobs have an anchor at minlength 20"""
    jobs = [p for _, p in lc.large_class_jobs(2)] + lc.corner_jobs()[:5]
    hit = 0
    for pair in jobs:
        anchors, T = mc.oracle_job(pair, 20)
        hit += 1 if anchors else 0
        assert T.upper() == (pair[0] + "$" + pair[1] + "$").upper().encode()
    assert 2 * hit > len(jobs)


def test_takes_shared_launch_rule_with_large():
    t = many.takes_shared_launch
    assert inspect.signature(t).parameters["large"].default is False
    assert inspect.signature(t).parameters["large_max"].default == many.LARGE_MAX >= 32768
    at, above = [b"A" * 1023, b"C" * 1023], [b"A" * 1024, b"C" * 1023]                   # 2048 and 2049 ranks
    assert t(at) and t(at, large=True) and not t(above) and t(above, large=True)
    assert not t(above, multi=True)
    cap, over = [b"A" * 16383, b"C" * 16383], [b"A" * 16384, b"C" * 16383]               # 32768 and 32769 ranks
    assert t(cap, large=True, large_max=32768) and not t(over, large=True, large_max=32768)
    assert t(over, large=True, large_max=32769) and not t(cap, large=False, large_max=32768)
    assert not t(above, large=True, large_max=2048)
    assert not t([b"A" * 1024, b"C" * 1023, b"G"], multi=True, large=True)               # three sequences above 2048 ranks: ordinary
    assert t([b"A" * 1000, b"C" * 1000, b"G"], multi=True, large=True)
    assert not t([b"A" * 1024, b"C\0" + b"C" * 1023], large=True)
    for (_, pair), want in zip(lc.large_class_jobs(1), [True] * len(lc.CLASSES)):
        assert t([s.encode() for s in pair], large=True) == want and not t([s.encode() for s in pair])


def test_shared_layout_round_trip_at_large_sizes():
    pairs = [(a.encode(), b.encode()) for a, b in lc.corner_jobs()[:5]] + [tuple(s.encode() for s in p) for _, p in lc.large_class_jobs(1)[:3]]
    text, abeg, bbeg = many.shared_layout(pairs)
    assert len(text) == sum(len(a) + len(b) + 2 for a, b in pairs)
    assert bbeg[0] == abeg[-1] + len(pairs[-1][0]) + 1
    for j, (a, b) in enumerate(pairs):
        alone = a + b"$" + b + b"$"
        la = len(a)
        for loc in list(range(0, len(alone), 37)) + [la - 1, la, la + 1, len(alone) - 1]:
            side, p = many.to_shared(loc, abeg[j], bbeg[j], la)
            assert text[p] == alone[loc]
            assert (side == 0) == (p < bbeg[0])
            assert many.to_local(p, side, abeg[j], bbeg[j], la) == loc
