"""align_many on the device (reveal_amd/many.py, csrc/rv_many.hip): every job's anchors and final text against the CPU oracle run
on that job ALONE (assemble + construct + align_bench) -- never against align_many itself."""
import random

import numpy as np
import pytest

import many_cases as mc
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

pytestmark = pytest.mark.gpu


def as_bytes(job):
    return [s.encode() if isinstance(s, str) else s for s in job]


def main_batch():
    """~400 class jobs (eligible for the shared launches), 20 pair jobs above 2048 ranks, jobs of three and five sequences"""
    jobs = [list(pair) for _, pair in mc.class_jobs(36)]
    jobs += [list(p) for p in mc.big_pairs(20)]
    jobs += mc.multi_jobs()
    random.Random(1).shuffle(jobs)
    return jobs


def expect_shared(jobs):
    return [len(j) == 2 and len(j[0]) + len(j[1]) + 2 <= 2048 for j in jobs]


def check_against_oracle(jobs, results, minl, sa64, which=None):
    bad = []
    for j in (range(len(jobs)) if which is None else which):
        anchors, T = mc.oracle_job(jobs[j], minl, 2, sa64)
        got = sorted((int(l), tuple(int(p) for p in pos)) for l, pos in results[j]["anchors"])
        if got != anchors or results[j]["T"].encode("latin-1") != T:
            bad.append((j, [len(s) for s in jobs[j]], got[:3], anchors[:3]))
    assert not bad, "%d jobs differ from the oracle, first: %r" % (len(bad), bad[:3])


@pytest.mark.parametrize("sa64", [False, True])
def test_every_job_equals_the_oracle_in_one_call(sa64):
    jobs = main_batch()
    results, info = many.align_many(jobs, minlength=20, minn=2, sa64=sa64, toupper=False)
    want = expect_shared(jobs)
    print("info", info)
    assert info["jobs"] == len(jobs) == len(results)
    assert info["shared"] == sum(want) and info["ordinary"] == len(jobs) - sum(want)      # no eligible job fell back, none was dropped
    assert info["shared"] > 0.9 * len(jobs)
    assert info["rounds"] == 1
    check_against_oracle(jobs, results, 20, sa64)
    assert sum(1 for r in results if r["anchors"]) > len(jobs) // 2


@pytest.mark.parametrize("sa64", [False, True])
def test_arrays_equal_the_stand_alone_construct(sa64):
    """RV_MANY_KEEP: SA and LCP of every shared-launch job = construct() of that job alone (pins the order of suffixes that tie through '$')"""
    jobs = [as_bytes(j) for j in main_batch()]
    want = expect_shared(jobs)
    b = many.Batch(sa64)
    b.option("RV_MANY_KEEP", 1)
    for j in jobs:
        b.add(j)
    b.run(20, 2)
    assert b.info()["shared"] == sum(want)
    bad = []
    for j, seqs in enumerate(jobs):
        if not want[j]:
            with pytest.raises(many.error):
                b.arrays(j)
            continue
        _, _, sa, lcp = mc.oracle_job([s.decode() for s in seqs], 20, 2, sa64, arrays=True)
        gsa, glcp = b.arrays(j)
        if not (np.array_equal(gsa, sa) and np.array_equal(glcp.astype(np.int64), lcp.astype(np.int64))):
            bad.append((j, [len(s) for s in seqs], int(np.argmax(gsa != sa)) if not np.array_equal(gsa, sa) else -1))
    assert not bad, "%d jobs' arrays differ, first: %r" % (len(bad), bad[:5])


@pytest.mark.parametrize("wave_max", [0, 100])
def test_size_class_switch_changes_nothing(wave_max):
    """RV_MANY_WAVE_MAX: every job through the workgroup-per-job build (0), or only the smallest through the wavefront build"""
    jobs = [as_bytes(list(pair)) for _, pair in mc.class_jobs(8, seed=99)]
    b = many.Batch(False)
    b.option("RV_MANY_WAVE_MAX", wave_max)
    results, info = many.align_many(jobs, 20, 2, toupper=False, batch=b)
    assert info["shared"] == len(jobs)
    check_against_oracle([[s.decode() for s in j] for j in jobs], results, 20, False)


def test_scale_launch_count_does_not_grow():
    big = [list(p) for p in mc.scale_jobs(20000)]
    small = big[:200]
    b = many.Batch(False)
    r_small, i_small = many.align_many(small, 20, 2, batch=b)
    r_big, i_big = many.align_many(big, 20, 2, batch=b)
    print("info", i_small, i_big)
    assert i_big["shared"] == 20000 and i_big["ordinary"] == 0 and i_small["shared"] == 200
    assert i_big["launches"] == i_small["launches"] and i_big["launches"] > 0
    assert i_big["rounds"] == i_small["rounds"] == 1
    sample = sorted(random.Random(17).sample(range(20000), 300))
    check_against_oracle(big, r_big, 20, False, which=sample)
    check_against_oracle(small, r_small, 20, False, which=range(0, 200, 7))


def test_rounds_split_a_large_text():
    """RV_MANY_ROUND: the text of a call is cut into rounds (what a call beyond the 32-bit library's position limit does)"""
    jobs = [list(p) for p in mc.scale_jobs(300, seed=4)]
    b = many.Batch(False)
    b.option("RV_MANY_ROUND", 20000)
    results, info = many.align_many(jobs, 20, 2, batch=b)
    assert info["rounds"] > 3 and info["shared"] == 300
    check_against_oracle(jobs, results, 20, False)


@pytest.mark.parametrize("minl", [1, 20])
def test_reuse_after_clear_and_minlength(minl):
    first = [list(pair) for _, pair in mc.class_jobs(3, seed=5)]
    second = [list(pair) for _, pair in mc.class_jobs(2, seed=6)] + [list(mc.big_pairs(1, seed=8)[0])] + mc.multi_jobs(seed=12)[:1]
    b = many.Batch(False)
    r1, i1 = many.align_many(first, minl, 2, toupper=False, batch=b)
    r2, i2 = many.align_many(second, minl, 2, toupper=False, batch=b)      # (align_many clears the batch first)
    assert i1["jobs"] == len(first) and i2["jobs"] == len(second) and i2["ordinary"] == 2
    check_against_oracle(first, r1, minl, False)
    check_against_oracle(second, r2, minl, False)


def test_refused_jobs():
    b = many.Batch(False)
    with pytest.raises(many.error, match="empty"):
        b.add([b"ACGT", b""])
    with pytest.raises(many.error, match="at least two"):
        b.add([b"ACGT"])
    with pytest.raises(many.error, match="non-ASCII"):
        b.add([b"ACGT", b"AC\xffT"])
    assert b.info()["jobs"] == 0
    b.add([b"ACGTACGTTTGACCA", b"ACGTACGTTTGACCA"])         # the batch is still usable
    b.run(5, 2)
    first, l, off, pos = b.anchors()
    assert first.tolist() == [0, 1] and l.tolist() == [15] and pos.tolist() == [0, 16]
    assert b.text(0) == b"acgtacgtttgacca$acgtacgtttgacca$"
    with pytest.raises(many.error, match="unknown option"):
        b.option("RV_NO_SUCH_SWITCH", 1)
