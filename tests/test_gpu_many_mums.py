"""GPU suite: `many.mums_many` / `Batch.scan` -- the MUM and multi-MUM lists of many small jobs in one call (csrc/rv_many_scan.hip) -- against the CPU
oracle on every job ALONE (tests/many_mums_cases.py oracle_matches), record for record and member for member, in the oracle's order.  Never against
the ordinary path alone, never against mums_many itself."""
import random

import numpy as np
import pytest

import many_cases as mc
import many_mums_cases as C
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

pytestmark = pytest.mark.gpu


def mixed_jobs():
    """the three batches, the corner jobs and the five ordinary jobs, shuffled"""
    jobs = C.multi_batch() + C.pair_batch() + C.wide_batch() + [s for _, s in C.corner_jobs()] + [s for _, s in C.ordinary_jobs()]
    random.Random(1).shuffle(jobs)
    return jobs


def as_bytes(jobs):
    return [[s.encode("latin-1") for s in seqs] for seqs in jobs]


def scan(jobs, minlength=20, minn=2, kind="auto", sa64=False, batch=None):
    return many.mums_many(jobs, minlength=minlength, minn=minn, kind=kind, sa64=sa64, toupper=False, batch=batch)


def check(jobs, matches, kind="auto", minl=20, minn=2):
    """every job's list equals the oracle's: the same records in the same order, the same members in the same order"""
    for j, seqs in enumerate(jobs):
        want = C.oracle_matches(seqs, kind, minl, minn)
        got = C.job_records(matches.arrays, j)
        assert got == want, (j, len(seqs), C.ranks(seqs), got[:3], want[:3])


def same_arrays(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("sa64", [False, True])
def test_every_job_equals_the_oracle_in_one_mixed_call(sa64):
    jobs = mixed_jobs()
    m, info = scan(jobs, sa64=sa64)
    check(jobs, m)
    shared = sum(1 for seqs in as_bytes(jobs) if many.takes_shared_scan(seqs))
    assert info["jobs"] == len(jobs) and info["shared"] == shared and info["ordinary"] == len(jobs) - shared == 5
    # the reference's shapes, on demand
    first = m.arrays[0]
    assert first[0] == 0 and first[-1] == len(m.arrays[1]) and len(m) == len(jobs)
    for j, seqs in enumerate(jobs):
        want = C.oracle_matches(seqs)
        if len(seqs) == 2:
            assert m[j] == [(l, (mem[0][1], mem[1][1]), 0) for l, _, mem in want]
        else:
            assert m[j] == [(l, n, mem) for l, n, mem in want]


@pytest.mark.parametrize("minl", [20, 3])
def test_corner_jobs(minl):
    jobs = [s for _, s in C.corner_jobs()] + [s for _, s in C.ordinary_jobs()]
    m, info = scan(jobs, minlength=minl)
    check(jobs, m, minl=minl)
    assert info["ordinary"] == 5 and info["shared"] == len(jobs) - 5


def test_getmums_and_getmultimums_on_the_same_jobs():
    jobs = C.multi_batch()[:20] + C.pair_batch() + C.wide_batch()[:2] + [s for _, s in C.corner_jobs()] + [s for _, s in C.ordinary_jobs()]
    for minl in (20, 1):
        m0, _ = scan(jobs, minlength=minl, kind="mums")
        check(jobs, m0, "mums", minl)                      # a job of k > 2: sample 0 against the rest
        m1, _ = scan(jobs, minlength=minl, kind="multimums")
        check(jobs, m1, "multimums", minl)                 # (members in SA order, pair jobs too)
        pairs = [j for j, s in enumerate(jobs) if len(s) == 2]
        for j in pairs:                                    # getmultimums on a pair job: getmums' records
            got = tuple((l, n, tuple(sorted(mem))) for l, n, mem in C.job_records(m1.arrays, j))
            assert got == C.oracle_matches(jobs[j], "mums", minl) == C.job_records(m0.arrays, j)
        assert all(m0[j] == [(l, (mem[0][1], mem[1][1]), 0) for l, _, mem in C.oracle_matches(jobs[j], "mums", minl)] for j in range(len(jobs)))


def test_minlength():
    jobs = C.multi_batch()[:10] + C.pair_batch()[:12] + [s for n, s in C.corner_jobs() if C.ranks(s) < 600] + [C.ordinary_jobs()[0][1]]
    res = {}
    for minl in (0, 1, 20, 1 << 20):
        res[minl], _ = scan(jobs, minlength=minl)
        check(jobs, res[minl], minl=minl)
    assert same_arrays(res[0].arrays, res[1].arrays)       # a match has l > 0
    first, l, n, off, so, pos = res[1 << 20].arrays        # above every LCP: empty lists, zero-length arrays
    assert not first.any() and len(first) == len(jobs) + 1 and len(l) == len(n) == len(so) == len(pos) == 0 and off.tolist() == [0]
    assert all(x == [] for x in res[1 << 20])


def test_minn():
    for fam in (C.multi_batch()[3], C.multi_batch()[9], C.wide_batch()[0], dict(C.ordinary_jobs())["three_by_1000"]):
        k = len(fam)
        jobs = [fam, C.NESTED_LAST]
        counts = []
        for minn in (2, 3, k, k + 1):
            m, _ = scan(jobs, minlength=5, minn=minn, kind="multimums")
            check(jobs, m, "multimums", 5, minn)
            counts.append(len(m[0]))
        assert counts[0] >= counts[1] >= counts[2] and counts[3] == 0, counts


def test_results_do_not_depend_on_the_path():
    jobs = mixed_jobs()
    b = many.Batch()
    shared, info = scan(jobs, batch=b)
    assert info["ordinary"] == 5
    b.option("RV_MANY_SCAN_ORDINARY", 1)
    ordinary, info = scan(jobs, batch=b)
    assert info["shared"] == 0 and info["ordinary"] == len(jobs) and info["rounds"] == 0
    assert same_arrays(shared.arrays, ordinary.arrays)
    check(jobs, shared)
    check(jobs, ordinary)
    b.option("RV_MANY_SCAN_ORDINARY", 0)
    for kind in ("mums", "multimums"):      # the ordinary path's own translations: getmums of k > 2, getmultimums of a pair index
        small = C.pair_batch()[:8] + C.multi_batch()[:4]
        s, _ = scan(small, minlength=5, kind=kind, batch=b)
        b.option("RV_MANY_SCAN_ORDINARY", 1)
        o, _ = scan(small, minlength=5, kind=kind, batch=b)
        b.option("RV_MANY_SCAN_ORDINARY", 0)
        assert same_arrays(s.arrays, o.arrays)
        check(small, o, kind, 5)


def test_rounds_and_size_classes():
    jobs = mixed_jobs()
    whole, info = scan(jobs)
    assert info["rounds"] == 1
    total = sum(C.ranks(s) for s in jobs if many.takes_shared_scan([x.encode("latin-1") for x in s]))
    b = many.Batch()
    b.option("RV_MANY_ROUND", total // 4)
    cut, info = scan(jobs, batch=b)
    assert info["rounds"] >= 3 and info["ordinary"] == 5
    assert same_arrays(whole.arrays, cut.arrays)
    b = many.Batch()
    b.option("RV_MANY_WAVE_MAX", 64)
    small_waves, _ = scan(jobs, batch=b)
    b.option("RV_MANY_WAVE_MAX", 512)
    large_waves, _ = scan(jobs, batch=b)
    assert same_arrays(whole.arrays, small_waves.arrays) and same_arrays(whole.arrays, large_waves.arrays)
    check(jobs, cut)


def test_launches_do_not_grow_with_the_jobs():
    """10 and 1000 jobs of one class in one round: the same launches (one build class, the count pass, three of the sum -- both rounds hold more
    than 2048 and fewer than 2^22 ranks --, the jobs' firsts, the write pass)"""
    rng = random.Random(4)
    jobs = []
    for _ in range(1000):
        a = mc.rnd(rng, 150)
        jobs.append([a, mc.mutate(rng, a, 0.02)])
    _, few = scan(jobs[:10])
    m, lots = scan(jobs)
    assert few["rounds"] == lots["rounds"] == 1 and few["shared"] == 10 and lots["shared"] == 1000
    assert few["launches"] == lots["launches"] == 7
    for j in range(0, 1000, 97):
        assert C.job_records(m.arrays, j) == C.oracle_matches(jobs[j])


def test_state_of_a_batch():
    jobs = C.pair_batch()[:10] + C.multi_batch()[:5]
    b = many.Batch()
    first_scan, _ = scan(jobs, batch=b)
    check(jobs, first_scan)
    with pytest.raises(many.error, match="scan"):
        b.text(0)
    with pytest.raises(many.error, match="scan"):
        b.anchors()
    b.run(20, 2)                                            # the same jobs: a scan leaves text and jobs untouched
    first, l, off, pos = b.anchors()
    ref, _ = many.align_many(as_bytes(jobs), toupper=False)
    for j in range(len(jobs)):      # (the order of a job's anchors is the leaf kernel's, launch by launch: the lists are compared sorted, as everywhere)
        assert sorted((int(l[k]), tuple(int(x) for x in pos[off[k]:off[k + 1]])) for k in range(first[j], first[j + 1])) == sorted(ref[j]["anchors"])
        assert b.text(j).decode("latin-1") == ref[j]["T"]
    with pytest.raises(many.error, match="run"):
        b.matches()
    b.scan(20, 2, "auto")
    assert same_arrays(first_scan.arrays, b.matches())
    assert b.info()["jobs"] == len(jobs)
    again, _ = scan(jobs, batch=b)                          # a reused Batch: the same result twice
    assert same_arrays(first_scan.arrays, again.arrays)
    b.clear()
    with pytest.raises(many.error):
        b.text(0)
    with pytest.raises(many.error):
        b.matches()


@pytest.mark.parametrize("sa64", [False, True])
def test_kept_arrays_after_a_scan(sa64):
    jobs = C.pair_batch()[:4] + C.multi_batch()[:4] + C.wide_batch()[:2]
    b = many.Batch(sa64)
    b.option("RV_MANY_KEEP", 1)
    m, _ = scan(jobs, sa64=sa64, batch=b)
    check(jobs, m)
    for j, seqs in enumerate(jobs):
        sa, lcp = b.arrays(j)
        osa, olcp = C.oracle_arrays(seqs)
        assert np.array_equal(sa.astype(np.int64), osa.astype(np.int64)) and np.array_equal(lcp.astype(np.int64), olcp.astype(np.int64)), j
