"""align_many with RV_MANY_LARGE on the device (reveal_amd/many.py, csrc/rv_many.hip, csrc/rv_many_large.hip): pair jobs above 2048 ranks
through the shared launches.  Every job's anchors, final text and (RV_MANY_KEEP) SA / LCP against the CPU oracle run on that job ALONE
(assemble + construct + align_bench) -- never against align_many itself."""
import functools
import random

import numpy as np
import pytest

import many_cases as mc
import many_large_cases as lc
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def ref(job, minl, sa64):
    """the oracle on one job (a tuple of str), computed once per process -> (anchors, T, SA, LCP)"""
    return mc.oracle_job(list(job), minl, 2, sa64, arrays=True)


def ranks(job):
    return sum(len(s) for s in job) + len(job)


def is_large(job):
    return len(job) == 2 and ranks(job) > many.LEAF_RANKS


def as_bytes(job):
    return [s.encode() for s in job]


def batch(sa64=False, large_max=32768, large_min=1, **more):
    b = many.Batch(sa64)
    b.option("RV_MANY_LARGE_MAX", large_max)
    b.option("RV_MANY_LARGE_MIN", large_min)
    for k, v in more.items():
        b.option(k, v)
    return b


def check_against_oracle(jobs, results, minl, sa64, which=None):
    bad = []
    for j in (range(len(jobs)) if which is None else which):
        anchors, T = ref(tuple(jobs[j]), minl, sa64)[:2]
        got = sorted((int(l), tuple(int(p) for p in pos)) for l, pos in results[j]["anchors"])
        if got != anchors or results[j]["T"].encode("latin-1") != T:
            bad.append((j, [len(s) for s in jobs[j]], got[:3], anchors[:3]))
    assert not bad, "%d jobs differ from the oracle, first: %r" % (len(bad), bad[:3])


def normal(results):
    """a job's anchors come in the order of the recursion's launches: sorted for a comparison"""
    return [(sorted(r["anchors"]), r["T"]) for r in results]


def check_arrays(b, jobs, which, sa64):
    bad = []
    for j in which:
        _, _, sa, lcp = ref(tuple(jobs[j]), 20, sa64)
        gsa, glcp = b.arrays(j)
        if not (np.array_equal(gsa, sa) and np.array_equal(glcp.astype(np.int64), lcp.astype(np.int64))):
            bad.append((j, [len(s) for s in jobs[j]], int(np.argmax(gsa != sa)) if not np.array_equal(gsa, sa) else -1))
    assert not bad, "%d jobs' arrays differ, first: %r" % (len(bad), bad[:5])


def main_batch():
    """40 class jobs of 2049 .. 6100 ranks, the corner jobs up to 20 000 ranks, 11 small pair jobs, jobs of three and five sequences"""
    jobs = [list(pair) for _, pair in lc.large_class_jobs(4)]
    jobs += [list(p) for p in lc.corner_jobs()[:-1]]
    jobs += [list(pair) for _, pair in mc.class_jobs(1)]
    jobs += mc.multi_jobs()
    random.Random(2).shuffle(jobs)
    return jobs


@pytest.mark.parametrize("sa64", [False, True])
def test_every_job_equals_the_oracle_in_one_call(sa64):
    jobs = main_batch()
    results, info = many.align_many(jobs, minlength=20, minn=2, sa64=sa64, toupper=False, batch=batch(sa64), large=True)
    print("info", info)
    want = sum(1 for j in jobs if len(j) == 2 and ranks(j) <= 32768)
    assert info["jobs"] == len(jobs) == len(results)
    assert info["shared"] == want and info["ordinary"] == len(jobs) - want == 5
    assert [many.takes_shared_launch(as_bytes(j), large=True, large_max=32768) for j in jobs].count(True) == want
    assert info["rounds"] == 2                                       # one of small jobs, one of large ones
    check_against_oracle(jobs, results, 20, sa64)
    large = [j for j in range(len(jobs)) if is_large(jobs[j])]
    assert len(large) == 46
    assert sum(1 for j in large if results[j]["anchors"]) > len(large) // 2


@pytest.mark.parametrize("sa64", [False, True])
def test_arrays_equal_the_stand_alone_construct(sa64):
    """RV_MANY_KEEP: SA and LCP of every large job = construct() of that job alone (pins ties through '$', the homopolymer and tandem
    orders, and the first job above 2048 ranks)"""
    jobs = main_batch()
    b = batch(sa64, RV_MANY_KEEP=1, RV_MANY_LARGE=1)
    for j in jobs:
        b.add(as_bytes(j))
    b.run(20, 2)
    large = [j for j in range(len(jobs)) if is_large(jobs[j])]
    assert b.info()["shared"] == len(jobs) - 5
    check_arrays(b, jobs, large, sa64)


def test_a_job_of_80002_ranks():
    """nothing of the build is 16 bits wide; above RV_MANY_LARGE_MAX the same job goes the ordinary way"""
    jobs = [list(lc.corner_jobs()[-1])]
    assert ranks(jobs[0]) == 80002
    b = batch(False, large_max=131072, RV_MANY_KEEP=1)
    results, info = many.align_many(jobs, 20, 2, toupper=False, batch=b, large=True)
    assert info["shared"] == 1 and info["ordinary"] == 0
    check_against_oracle(jobs, results, 20, False)
    check_arrays(b, jobs, [0], False)
    assert results[0]["anchors"]
    results, info = many.align_many(jobs, 20, 2, toupper=False, batch=batch(False, large_max=32768), large=True)
    assert info["shared"] == 0 and info["ordinary"] == 1
    check_against_oracle(jobs, results, 20, False)


def test_switch_off_against_on():
    jobs = [list(pair) for _, pair in lc.large_class_jobs(1, seed=77)] + [list(p) for p in lc.corner_jobs()[:5]]
    jobs += [list(pair) for _, pair in mc.class_jobs(1, seed=78)]
    nlarge = sum(1 for j in jobs if is_large(j))
    assert nlarge == 14
    r_off, i_off = many.align_many(jobs, 20, 2, toupper=False, batch=batch(), large=False)
    r_on, i_on = many.align_many(jobs, 20, 2, toupper=False, batch=batch(), large=True)
    r_none, i_none = many.align_many(jobs, 20, 2, toupper=False, batch=batch())          # off unless asked for
    assert i_on["shared"] == len(jobs) and i_on["ordinary"] == 0
    assert i_off["shared"] == i_on["shared"] - nlarge and i_off["ordinary"] == nlarge
    assert (i_none["shared"], i_none["ordinary"], i_none["rounds"], i_none["launches"]) == (i_off["shared"], i_off["ordinary"], i_off["rounds"], i_off["launches"])
    assert normal(r_off) == normal(r_on) == normal(r_none)
    check_against_oracle(jobs, r_on, 20, False)
    check_against_oracle(jobs, r_off, 20, False)
    # fewer large jobs than RV_MANY_LARGE_MIN: the ordinary way
    five = [j for j in jobs if is_large(j)][:5] + [j for j in jobs if not is_large(j)][:3]
    r_min, i_min = many.align_many(five, 20, 2, toupper=False, batch=batch(large_min=1000), large=True)
    assert i_min["shared"] == 3 and i_min["ordinary"] == 5
    check_against_oracle(five, r_min, 20, False)
    r_min, i_min = many.align_many(five, 20, 2, toupper=False, batch=batch(large_min=5), large=True)
    assert i_min["shared"] == 8 and i_min["ordinary"] == 0
    check_against_oracle(five, r_min, 20, False)


def test_launch_count_does_not_grow_with_the_jobs():
    once = [list(pair) for _, pair in lc.large_class_jobs(3)]
    tenfold = once * 10
    b = batch()
    r1, i1 = many.align_many(once, 20, 2, toupper=False, batch=b, large=True)
    r10, i10 = many.align_many(tenfold, 20, 2, toupper=False, batch=b, large=True)
    print("info", i1, i10)
    assert i1["shared"] == len(once) and i10["shared"] == len(tenfold) and i1["ordinary"] == i10["ordinary"] == 0
    assert i10["launches"] == i1["launches"] and i1["launches"] > 0
    assert i10["rounds"] == i1["rounds"] == 1
    check_against_oracle(once, r1, 20, False)
    check_against_oracle(tenfold, r10, 20, False, which=sorted(random.Random(3).sample(range(len(tenfold)), 60)))


def test_rounds_split_the_large_jobs():
    jobs = [list(pair) for _, pair in lc.large_class_jobs(4, seed=9)]
    rng = random.Random(10)
    a = mc.rnd(rng, 20000)
    jobs.append([a, mc.mutate(rng, a, 0.01)])                        # 40 002 ranks: larger than a round
    b = batch(large_max=1 << 20, RV_MANY_ROUND=30000)
    results, info = many.align_many(jobs, 20, 2, toupper=False, batch=b, large=True)
    print("info", info)
    assert info["rounds"] > 3 and info["shared"] == 40 and info["ordinary"] == 1
    check_against_oracle(jobs, results, 20, False)


def test_reuse_after_clear_and_minlength():
    first = [list(pair) for _, pair in mc.class_jobs(1, seed=5)] + [list(pair) for _, pair in lc.large_class_jobs(1, seed=6)] + mc.multi_jobs(seed=12)[:3]
    second = [list(pair) for _, pair in lc.large_class_jobs(1, seed=7)][:6] + [list(pair) for _, pair in mc.class_jobs(1, seed=8)][:5] + mc.multi_jobs(seed=13)[3:]
    b = batch()
    for minl in (1, 20):
        r1, i1 = many.align_many(first, minl, 2, toupper=False, batch=b, large=True, multi=True)
        r2, i2 = many.align_many(second, minl, 2, toupper=False, batch=b, large=True, multi=True)      # (align_many clears the batch first)
        assert i1["shared"] == i1["jobs"] == len(first) and i2["shared"] == i2["jobs"] == len(second)
        assert i1["ordinary"] == i2["ordinary"] == 0
        check_against_oracle(first, r1, minl, False)
        check_against_oracle(second, r2, minl, False)
