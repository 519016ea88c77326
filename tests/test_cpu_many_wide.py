"""RV_MANY_WIDE without a device: the job generator of tests/test_gpu_many_wide.py (from the CPU oracle alone: its jobs HAVE anchors, so the
device tests cannot pass by anchoring nothing) and the eligibility rule with the new keyword."""
import inspect

import many_cases as mc
import many_large_multi_cases as lm
import many_multi_cases as mm
import many_wide_cases as mw
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many


def as_bytes(job):
    return [s.encode() for s in job]


def test_generator_is_deterministic_and_in_range():
    assert mw.class_jobs(16) == mw.class_jobs(16) and mw.sites_jobs(5) == mw.sites_jobs(5) and mw.large_jobs(4) == mw.large_jobs(4)
    assert mw.short_jobs(4) == mw.short_jobs(4) and mw.scale_jobs(30) == mw.scale_jobs(30) and mw.corner_jobs() == mw.corner_jobs()
    assert mw.class_jobs(8, seed=5) != mw.class_jobs(8, seed=6)
    assert mw.K_VALUES == (17, 24, 32, 33, 48, 64) and many.WIDE_KMAX == 64 and many.MULTI_KMAX == 16
    seen = set()
    for cls, k, seqs in mw.class_jobs(24):
        assert len(seqs) == k and all(len(s) >= 1 for s in seqs), cls
        assert mw.ranks(seqs) <= mw.MAX_RANKS == many.LEAF_RANKS, (cls, k, mw.ranks(seqs))                   # every "small" job
        assert many.takes_shared_launch(as_bytes(seqs), wide=True)
        assert not many.takes_shared_launch(as_bytes(seqs), multi=True, large=True, large_multi=True)
        seen.add((cls, k))
    assert len(seen) == len(mw.CLASSES) * len(mw.K_VALUES)
    for k, seqs in mw.sites_jobs(20):
        assert len(seqs) == k and mw.ranks(seqs) <= mw.MAX_RANKS and len({len(s) for s in seqs}) == 1
        assert 1 < len(set(seqs)) or k < 2                                                                  # a variant site in a proper subset
    for cls, k, seqs in mw.large_jobs(8):
        assert len(seqs) == k and mw.LARGE_RANKS[0] <= mw.ranks(seqs) <= mw.LARGE_RANKS[1], (cls, k, mw.ranks(seqs))      # every "large" one
        assert mw.ranks(seqs) > many.LEAF_RANKS and many.takes_shared_launch(as_bytes(seqs), wide=True)
    assert {k for _, k, _ in mw.large_jobs(8)} == {17, 33, 64}
    assert all(mw.ranks(j) <= 600 for j in mw.short_jobs(12)) and {len(j) for j in mw.short_jobs(12)} == {17, 33, 64}
    assert all(mw.ranks(j) <= mw.MAX_RANKS for j in mw.scale_jobs(200)) and {len(j) for j in mw.scale_jobs(200)} == set(mw.K_VALUES)


def test_corner_jobs():
    c = mw.corner_jobs()
    assert tuple(n for n, _, _ in c) == mw.CORNER_NAMES
    assert [(len(s), mw.ranks(s)) for _, s, _ in c] == [(17, 34), (64, 128), (17, 680), (64, 2048), (64, 2049), (65, 1365), (16, 976)]
    assert [kind for _, _, kind in c] == ["small", "small", "small", "small", "large", "never", "other"]
    t = many.takes_shared_launch
    assert [t(as_bytes(s), wide=True) for _, s, _ in c] == [True, True, True, True, True, False, False]
    assert [t(as_bytes(s), multi=True, wide=True) for _, s, _ in c][-2:] == [False, True]      # 16 sequences: where it went before
    assert not any(t(as_bytes(s)) for _, s, _ in c)
    assert dict((n, s) for n, s, _ in c)["k17"] == dict((n, s) for n, s, _ in mm.corner_jobs())["k17"]


def test_sites_jobs_have_anchors():
    """the CPU oracle alone, on the committed generator and seeds: at minlength 12 at least 3 of every 4 "sites" jobs per k have an anchor; at
    minlength 1 at least a third of them have three or more"""
    for k in mw.K_VALUES:
        jobs = [seqs for kk, seqs in mw.sites_jobs(20) if kk == k]
        hit = sum(1 for j in jobs if mw.oracle_job(j, 12)[0])
        three = sum(1 for j in jobs if len(mw.oracle_job(j, 1)[0]) >= 3)
        print("k", k, "jobs", len(jobs), "anchored at minlength 12:", hit, "three or more anchors at minlength 1:", three)
        assert len(jobs) == 20 and 4 * hit >= 3 * len(jobs), (k, hit)
        assert 3 * three >= len(jobs), (k, three)
        for j in jobs:
            anchors, T = mw.oracle_job(j, 12)
            assert T.upper() == "".join(s + "$" for s in j).upper().encode()
            assert all(2 <= len(pos) <= k for _, pos in anchors)


def test_dropout_jobs_anchor_fewer_than_k_samples():
    """at least one dropout job per k has an anchor on fewer than k samples, at the minlength 12 of the device tests"""
    for k in mw.K_VALUES:
        jobs = [seqs for cls, kk, seqs in mw.class_jobs(24) if kk == k and cls == "dropout"]
        fewer = sum(1 for j in jobs if any(len(pos) < k for _, pos in mw.oracle_job(j, 12)[0]))
        print("k", k, "dropout jobs", len(jobs), "with an anchor on fewer than k samples:", fewer)
        assert len(jobs) == 3 and fewer >= 1, (k, fewer)


def test_takes_shared_launch_rule_with_wide():
    t = many.takes_shared_launch
    assert inspect.signature(t).parameters["wide"].default is False
    assert inspect.signature(many.align_many).parameters["wide"].default is None
    k16, k17, k64, k65 = [b"ACGT" * 5] * 16, [b"ACGT" * 5] * 17, [b"ACGT" * 5] * 64, [b"ACGT" * 5] * 65
    assert not t(k17) and not t(k17, multi=True, large=True, large_multi=True) and t(k17, wide=True)
    assert t(k64, wide=True) and not t(k65, wide=True) and not t(k65, multi=True, large=True, large_multi=True, wide=True)
    assert not t(k16, wide=True) and t(k16, multi=True) and t(k16, multi=True, wide=True)      # RV_MANY_MULTI's class is untouched
    assert not t([b"A", b"C"] * 9 + [b"G\0"], wide=True)
    at, above = [b"A" * 31] * 64, [b"A" * 31] * 63 + [b"A" * 32]                               # 2048 and 2049 ranks
    assert t(at, wide=True) and t(above, wide=True) and not t(above, large_multi=True) and not t(above, wide=True, large_max=2048)
    assert t([b"A" * 2047] * 64, wide=True) and not t([b"A" * 2048] * 64, wide=True)           # 2^17 ranks, and above the default RV_MANY_LARGE_MAX
    assert t([b"A" * 2048] * 64, wide=True, large_max=1 << 18)
    # with the default the function answers exactly as before, on the jobs of the other classes' generators: today's rule, written out
    def before(seqs, multi=False, large=False, large_max=many.LARGE_MAX, large_multi=False):
        k, ranks = len(seqs), sum(len(s) for s in seqs) + len(seqs)
        if not (2 <= k <= 16) or any(b"\0" in s for s in seqs):
            return False
        if ranks <= 2048:
            return k == 2 or bool(multi)
        return ranks <= large_max and bool(large if k == 2 else large_multi)
    jobs = [seqs for _, _, seqs in mm.class_jobs(3)] + [seqs for _, seqs, _ in mm.corner_jobs()]
    jobs += [seqs for _, _, seqs in lm.class_jobs(2)] + lm.corner_jobs() + [list(p) for _, p in mc.class_jobs(1)] + [list(p) for p in mc.big_pairs(2)]
    assert {len(j) for j in jobs} >= {2, 3, 16, 17}
    for j in jobs:
        seqs = as_bytes(j)
        for multi in (False, True):
            for large in (False, True):
                for large_multi in (False, True):
                    for large_max in (many.LARGE_MAX, 32768):
                        kw = dict(multi=multi, large=large, large_max=large_max, large_multi=large_multi)
                        assert t(seqs, **kw) == t(seqs, wide=False, **kw) == before(seqs, **kw), (len(j), kw)
                        if len(j) <= 16:
                            assert t(seqs, wide=True, **kw) == before(seqs, **kw)
