"""align_many with RV_MANY_LARGE_MULTI on the device (reveal_amd/many.py, csrc/rv_many.hip, csrc/rv_many_large.hip): jobs of 3 .. 16 sequences
above 2048 ranks through the shared launches, sample-major rounds of mixed k.  Every job's anchors, final text and (RV_MANY_KEEP) SA / LCP against
the CPU oracle run on that job ALONE (many_multi_cases.oracle_job: assemble + construct + align_bench) -- never against align_many itself."""
import random

import numpy as np
import pytest

import many_cases as mc
import many_large_cases as lc
import many_large_multi_cases as lm
import many_multi_cases as mm
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

pytestmark = pytest.mark.gpu


def ranks(job):
    return sum(len(s) for s in job) + len(job)


def is_new_class(job, large_max=32768):
    return 3 <= len(job) <= 16 and many.LEAF_RANKS < ranks(job) <= large_max


def as_bytes(job):
    return [s.encode() for s in job]


def batch(sa64=False, large_max=32768, large_min=1, multi_min=1, **more):
    b = many.Batch(sa64)
    b.option("RV_MANY_LARGE_MAX", large_max)
    b.option("RV_MANY_LARGE_MIN", large_min)
    b.option("RV_MANY_LARGE_MULTI_MIN", multi_min)
    for k, v in more.items():
        b.option(k, v)
    return b


def check_against_oracle(jobs, results, minl, sa64, which=None, minn=2):
    bad = []
    for j in (range(len(jobs)) if which is None else which):
        anchors, T = mm.oracle_job(jobs[j], minl, minn, sa64, arrays=True)[:2]
        got = sorted((int(l), tuple(int(p) for p in pos)) for l, pos in results[j]["anchors"])
        if got != anchors or results[j]["T"].encode("latin-1") != T:
            bad.append((j, [len(s) for s in jobs[j]], got[:3], anchors[:3]))
    assert not bad, "%d jobs differ from the oracle, first: %r" % (len(bad), bad[:3])


def check_arrays(b, jobs, which, sa64):
    bad = []
    for j in which:
        _, _, sa, lcp = mm.oracle_job(jobs[j], 20, 2, sa64, arrays=True)
        gsa, glcp = b.arrays(j)
        if not (np.array_equal(gsa, sa) and np.array_equal(glcp.astype(np.int64), lcp.astype(np.int64))):
            bad.append((j, [len(s) for s in jobs[j]], int(np.argmax(gsa != sa)) if not np.array_equal(gsa, sa) else -1))
    assert not bad, "%d jobs' arrays differ, first: %r" % (len(bad), bad[:5])


def normal(results):
    """a job's anchors come in the order of the recursion's launches: sorted for a comparison"""
    return [(sorted(r["anchors"]), r["T"]) for r in results]


def main_batch():
    """16 class jobs of 2049 .. 6100 ranks over k = 3 .. 16, the corner jobs up to 20 001 ranks (one of them, of 2048 ranks, is not of the new
    class), 11 small pair jobs, five small jobs of three and more sequences, three pair jobs above 2048 ranks"""
    jobs = [seqs for _, _, seqs in lm.class_jobs(2)]
    jobs += lm.corner_jobs()[:-1]
    jobs += [list(pair) for _, pair in mc.class_jobs(1)]
    jobs += mm.small_jobs(5)
    jobs += [list(p) for p in mc.big_pairs(3)]
    random.Random(2).shuffle(jobs)
    return jobs


@pytest.mark.parametrize("sa64", [False, True])
def test_every_job_equals_the_oracle_in_one_call(sa64):
    jobs = main_batch()
    results, info = many.align_many(jobs, minlength=20, minn=2, sa64=sa64, toupper=False, batch=batch(sa64), large_multi=True)
    print("info", info)
    new = [j for j in range(len(jobs)) if is_new_class(jobs[j])]
    assert len(new) == 16 + 6 and {len(jobs[j]) for j in new} == {3, 4, 5, 8, 16}
    want = [many.takes_shared_launch(as_bytes(j), large_multi=True, large_max=32768) for j in jobs].count(True)
    assert want == len(new) + 11
    assert info["jobs"] == len(jobs) == len(results)
    assert info["shared"] == want and info["ordinary"] == len(jobs) - want == 1 + 5 + 3
    assert info["rounds"] == 2                                       # one of small pair jobs, one of the new class with every k in it
    check_against_oracle(jobs, results, 20, sa64)
    assert sum(1 for j in new if results[j]["anchors"]) > len(new) // 2


@pytest.mark.parametrize("sa64", [False, True])
def test_arrays_equal_the_stand_alone_construct(sa64):
    """RV_MANY_KEEP: SA and LCP of every job of the new class = construct() of that job alone (pins ties through '$' among k identical alleles,
    the homopolymer and tandem orders, the first job above 2048 ranks and the job of 16 sequences)"""
    jobs = main_batch()
    b = batch(sa64, RV_MANY_KEEP=1, RV_MANY_LARGE_MULTI=1)
    for j in jobs:
        b.add(as_bytes(j))
    b.run(20, 2)
    new = [j for j in range(len(jobs)) if is_new_class(jobs[j])]
    assert b.info()["shared"] == len(new) + 11
    check_arrays(b, jobs, new, sa64)


def test_a_job_of_66003_ranks():
    """nothing of the build is 16 bits wide; above RV_MANY_LARGE_MAX the same job goes the ordinary way"""
    jobs = [lm.corner_jobs()[-1]]
    assert ranks(jobs[0]) == 66003 and len(jobs[0]) == 3
    b = batch(False, large_max=131072, RV_MANY_KEEP=1)
    results, info = many.align_many(jobs, 20, 2, toupper=False, batch=b, large_multi=True)
    assert info["shared"] == 1 and info["ordinary"] == 0
    check_against_oracle(jobs, results, 20, False)
    check_arrays(b, jobs, [0], False)
    assert results[0]["anchors"]
    results, info = many.align_many(jobs, 20, 2, toupper=False, batch=batch(False, large_max=32768), large_multi=True)
    assert info["shared"] == 0 and info["ordinary"] == 1
    check_against_oracle(jobs, results, 20, False)


def test_switch_off_against_on():
    jobs = [seqs for _, _, seqs in lm.class_jobs(1, seed=77)] + lm.corner_jobs()[:6]
    jobs += [list(pair) for _, pair in mc.class_jobs(1, seed=78)][:6] + mm.small_jobs(3, seed=79) + [list(p) for p in mc.big_pairs(2, seed=80)]
    nnew = sum(1 for j in jobs if is_new_class(j))
    assert nnew == 8 + 5
    r_off, i_off = many.align_many(jobs, 20, 2, toupper=False, batch=batch(), large_multi=False)
    r_on, i_on = many.align_many(jobs, 20, 2, toupper=False, batch=batch(), large_multi=True)
    r_none, i_none = many.align_many(jobs, 20, 2, toupper=False, batch=batch())          # off unless asked for
    assert i_on["shared"] == 6 + nnew and i_on["ordinary"] == len(jobs) - 6 - nnew == 1 + 3 + 2
    assert i_off["shared"] == 6 and i_off["ordinary"] == len(jobs) - 6
    assert (i_none["shared"], i_none["ordinary"], i_none["rounds"], i_none["launches"]) == (i_off["shared"], i_off["ordinary"], i_off["rounds"], i_off["launches"])
    assert normal(r_off) == normal(r_on) == normal(r_none)
    check_against_oracle(jobs, r_on, 20, False)
    check_against_oracle(jobs, r_off, 20, False)
    # RV_MANY_LARGE alone leaves these jobs ordinary (and takes the two pair jobs above 2048 ranks)
    r_l, i_l = many.align_many(jobs, 20, 2, toupper=False, batch=batch(), large=True)
    assert i_l["shared"] == 6 + 2 and i_l["ordinary"] == len(jobs) - 8
    assert normal(r_l) == normal(r_on)
    # fewer such jobs than RV_MANY_LARGE_MULTI_MIN (this class has a threshold of its own: DESIGN.md 3j): the ordinary way; the count is of these
    # jobs alone, whatever pair jobs the call holds, and RV_MANY_LARGE_MIN does not touch them
    five = [j for j in jobs if is_new_class(j)][:5] + [j for j in jobs if len(j) == 2][:8]
    assert sum(1 for j in five if len(j) == 2 and ranks(j) > 2048) == 2
    r_min, i_min = many.align_many(five, 20, 2, toupper=False, batch=batch(multi_min=6), large_multi=True)
    assert i_min["shared"] == 6 and i_min["ordinary"] == 5 + 2
    check_against_oracle(five, r_min, 20, False)
    b = many.Batch(False)                                             # the default threshold is above five
    b.option("RV_MANY_LARGE_MAX", 32768)
    r_min, i_min = many.align_many(five, 20, 2, toupper=False, batch=b, large_multi=True)
    assert i_min["shared"] == 6 and i_min["ordinary"] == 5 + 2
    r_min, i_min = many.align_many(five, 20, 2, toupper=False, batch=batch(large_min=1000, multi_min=5), large_multi=True)
    assert i_min["shared"] == 6 + 5 and i_min["ordinary"] == 2
    check_against_oracle(five, r_min, 20, False)


@pytest.mark.parametrize("minn", [2, 3, 5])
def test_minn_and_subsets(minn):
    """families of five of class dropout: one sample runs out, so sub-indices go on with fewer samples than the job's k = 5 and than the round's
    K = 8 (a job of eight sequences shares the round)"""
    jobs = [lm.make_large_family("dropout", random.Random(500 + x), 5) for x in range(4)] + [lm.sized_job(random.Random(510), 8, 2500)]
    results, info = many.align_many(jobs, 20, minn, toupper=False, batch=batch(), large_multi=True)
    assert info["shared"] == len(jobs) and info["ordinary"] == 0 and info["rounds"] == 1
    check_against_oracle(jobs, results, 20, False, minn=minn)
    sizes = {len(pos) for r in results[:4] for _, pos in r["anchors"]}
    print("members per anchor", sorted(sizes))
    assert 5 in sizes and all(minn <= s <= 5 for s in sizes)
    if minn < 5:
        assert min(sizes) < 5


def test_launch_count_does_not_grow_with_the_jobs():
    once = [seqs for _, _, seqs in lm.class_jobs(2, seed=21)]
    tenfold = once * 10
    b = batch()
    r1, i1 = many.align_many(once, 20, 2, toupper=False, batch=b, large_multi=True)
    r10, i10 = many.align_many(tenfold, 20, 2, toupper=False, batch=b, large_multi=True)
    print("info", i1, i10)
    assert i1["shared"] == len(once) and i10["shared"] == len(tenfold) and i1["ordinary"] == i10["ordinary"] == 0
    assert i10["launches"] == i1["launches"] and i1["launches"] > 0
    assert i10["rounds"] == i1["rounds"] == 1
    check_against_oracle(once, r1, 20, False)
    check_against_oracle(tenfold, r10, 20, False, which=sorted(random.Random(3).sample(range(len(tenfold)), 60)))


def test_rounds_split_the_jobs():
    jobs = [seqs for _, _, seqs in lm.class_jobs(3, seed=9)]
    rng = random.Random(10)
    a = mc.rnd(rng, 13000)
    jobs.append([mc.mutate(rng, a, 0.01) for _ in range(3)])         # 39 003 ranks: larger than a round
    b = batch(large_max=1 << 20, RV_MANY_ROUND=30000)
    results, info = many.align_many(jobs, 20, 2, toupper=False, batch=b, large_multi=True)
    print("info", info)
    assert info["rounds"] > 3 and info["shared"] == 24 and info["ordinary"] == 1
    check_against_oracle(jobs, results, 20, False)


def test_reuse_with_every_switch():
    """one Batch, two different calls, RV_MANY_MULTI, RV_MANY_LARGE and RV_MANY_LARGE_MULTI on: nothing is ordinary.  (minlength 1 takes a level
    per few bases of a job: those jobs stay at about 2100 ranks)"""
    rng = random.Random(31)
    pairs = [list(p) for _, p in mc.class_jobs(1, seed=5)]
    small = {1: lm.sized_jobs(5, lo=2049, hi=2120, seed=32), 20: [seqs for _, _, seqs in lm.class_jobs(1, seed=33)]}
    big_pair = {1: [[mc.rnd(rng, 1030), mc.rnd(rng, 1040)]], 20: [list(p) for _, p in lc.large_class_jobs(1, seed=6)][:4]}
    for minl in (1, 20):
        first = pairs[:6] + small[minl][:3] + mm.small_jobs(4, seed=34) + big_pair[minl]
        second = small[minl][3:] + pairs[6:] + mm.small_jobs(3, seed=35) + big_pair[minl][:1]
        b = batch()
        r1, i1 = many.align_many(first, minl, 2, toupper=False, batch=b, multi=True, large=True, large_multi=True)
        r2, i2 = many.align_many(second, minl, 2, toupper=False, batch=b)      # (align_many clears the batch first; the switches stay)
        print("info", minl, i1, i2)
        assert i1["shared"] == i1["jobs"] == len(first) and i2["shared"] == i2["jobs"] == len(second)
        assert i1["ordinary"] == i2["ordinary"] == 0
        check_against_oracle(first, r1, minl, False)
        check_against_oracle(second, r2, minl, False)
