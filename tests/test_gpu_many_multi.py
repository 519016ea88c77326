"""align_many with RV_MANY_MULTI on the device (reveal_amd/many.py, csrc/rv_many.hip, csrc/rv_leaf_multi.hip): jobs of three and
more sequences through the shared launches.  Every job's anchors and final text are checked against the CPU oracle run on that
job ALONE (assemble + construct + align_bench) -- never against the ordinary path or align_many itself."""
import random

import numpy as np
import pytest

import many_cases as mc
import many_multi_cases as mm
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

pytestmark = pytest.mark.gpu


def as_bytes(job):
    return [s.encode() if isinstance(s, str) else s for s in job]


def main_batch():
    """~225 class jobs of 3 .. 16 sequences, the corner jobs (two of them ordinary), 44 pair jobs, the ordinary jobs of many_cases"""
    jobs = [seqs for _, _, seqs in mm.class_jobs(25)]
    jobs += [seqs for _, seqs, _ in mm.corner_jobs()]
    jobs += [list(pair) for _, pair in mc.class_jobs(4)]
    jobs += [list(p) for p in mc.big_pairs(2)] + mc.multi_jobs()
    random.Random(2).shuffle(jobs)
    return jobs


def shared_with(jobs, multi):
    return [many.takes_shared_launch(as_bytes(j), multi=multi) for j in jobs]


def check_against_oracle(jobs, results, minl, sa64, minn=2, which=None):
    bad = []
    total_l = nanch = 0
    for j in (range(len(jobs)) if which is None else which):
        anchors, T = mm.oracle_job(jobs[j], minl, minn, sa64)
        got = sorted((int(l), tuple(int(p) for p in pos)) for l, pos in results[j]["anchors"])
        if got != anchors or results[j]["T"].encode("latin-1") != T:
            bad.append((j, [len(s) for s in jobs[j]], got[:3], anchors[:3]))
        total_l += sum(l for l, _ in anchors)
        nanch += len(anchors)
    assert not bad, "%d jobs differ from the oracle, first: %r" % (len(bad), bad[:3])
    return nanch, total_l


@pytest.mark.parametrize("sa64", [False, True])
def test_every_job_equals_the_oracle_in_one_call(sa64):
    jobs = main_batch()
    results, info = many.align_many(jobs, minlength=20, minn=2, sa64=sa64, toupper=False, multi=True)
    want = shared_with(jobs, True)
    print("info", info)
    assert info["jobs"] == len(jobs) == len(results)
    assert sum(1 for j, w in zip(jobs, want) if w and len(j) > 2) > 200 and sum(1 for j, w in zip(jobs, want) if not w) >= 5
    assert info["shared"] == sum(want) and info["ordinary"] == len(jobs) - sum(want)      # no eligible job fell back, none was dropped
    nanch, total_l = check_against_oracle(jobs, results, 20, sa64)
    assert sum(1 for r in results if r["anchors"]) > len(jobs) // 2
    assert info["stats"]["splits"] == nanch and info["stats"]["anchored_bp"] == total_l


def test_results_do_not_depend_on_the_switch():
    jobs = main_batch()
    results, info = many.align_many(jobs, minlength=20, minn=2, toupper=False, multi=False)
    want = shared_with(jobs, False)
    assert info["shared"] == sum(want) == sum(1 for j in jobs if len(j) == 2 and mm.ranks(j) <= 2048)
    assert info["ordinary"] == len(jobs) - sum(want)      # every job of three and more sequences among them
    check_against_oracle(jobs, results, 20, False)


@pytest.mark.parametrize("sa64", [False, True])
def test_arrays_equal_the_stand_alone_construct(sa64):
    """RV_MANY_KEEP: SA and LCP of every shared job = construct() of that job alone, with the suffixes that tie through '$'
    between identical alleles of several samples in the stand-alone order"""
    jobs = [seqs for _, _, seqs in mm.class_jobs(10, classes=("identical", "dup", "snp", "tandem", "len1"))]
    jobs += [seqs for _, seqs, _ in mm.corner_jobs()] + [list(pair) for _, pair in mc.class_jobs(1)]
    want = shared_with(jobs, True)
    b = many.Batch(sa64)
    b.option("RV_MANY_KEEP", 1)
    b.option("RV_MANY_MULTI", 1)
    for j in jobs:
        b.add(as_bytes(j))
    b.run(20, 2)
    assert b.info()["shared"] == sum(want)
    bad = []
    for j, seqs in enumerate(jobs):
        if not want[j]:
            with pytest.raises(many.error):
                b.arrays(j)
            continue
        _, _, sa, lcp = mm.oracle_job(seqs, 20, 2, sa64, arrays=True)
        gsa, glcp = b.arrays(j)
        if not (np.array_equal(gsa, sa) and np.array_equal(glcp.astype(np.int64), lcp.astype(np.int64))):
            bad.append((j, [len(s) for s in seqs], int(np.argmax(gsa != sa)) if not np.array_equal(gsa, sa) else -1))
    assert not bad, "%d jobs' arrays differ, first: %r" % (len(bad), bad[:5])


def test_minn():
    """minn 2, 3, k and k + 1: a sub-index of fewer than minn samples anchors nothing; k + 1: nothing at all"""
    fams = mm.class_jobs(10, seed=77, classes=("dropout", "snp"))
    for sel in ("2", "3", "k", "k+1"):
        groups = {}
        for _, k, seqs in fams:
            groups.setdefault({"2": 2, "3": 3, "k": k, "k+1": k + 1}[sel], []).append(seqs)
        for minn, jobs in sorted(groups.items()):
            results, info = many.align_many(jobs, 20, minn, toupper=False, multi=True)
            assert info["shared"] == len(jobs)
            nanch, _ = check_against_oracle(jobs, results, 20, False, minn=minn)
            if sel == "k+1":
                assert nanch == 0


@pytest.mark.parametrize("minl", [1, 20])
@pytest.mark.parametrize("stage", [256, 2])
def test_minlength_and_the_direct_anchor_path(minl, stage):
    """minlength 1 on jobs of at most ~200 ranks (up to eight anchors per job: a match has to be unique on every sample);
    RV_MANY_STAGE 2: all but two anchors of a job leave the workgroup directly, not through its staging"""
    jobs = mm.small_jobs(60)
    b = many.Batch(False)
    b.option("RV_MANY_STAGE", stage)
    results, info = many.align_many(jobs, minl, 2, toupper=False, batch=b, multi=True)
    assert info["shared"] == len(jobs) and info["ordinary"] == 0
    nanch, total_l = check_against_oracle(jobs, results, minl, False)
    assert info["stats"]["splits"] == nanch and info["stats"]["anchored_bp"] == total_l
    if minl == 1:
        assert max(len(r["anchors"]) for r in results) > 2 * 2


@pytest.mark.parametrize("wave_max", [0, 100])
def test_size_class_switch_changes_nothing(wave_max):
    jobs = [seqs for _, _, seqs in mm.class_jobs(5, seed=99)]
    b = many.Batch(False)
    b.option("RV_MANY_WAVE_MAX", wave_max)
    results, info = many.align_many(jobs, 20, 2, toupper=False, batch=b, multi=True)
    assert info["shared"] == len(jobs)
    check_against_oracle(jobs, results, 20, False)


def test_rounds_split_a_large_text():
    jobs = mm.scale_jobs(300, seed=4)
    b = many.Batch(False)
    b.option("RV_MANY_ROUND", 20000)
    results, info = many.align_many(jobs, 20, 2, batch=b, multi=True)
    assert info["rounds"] > 3 and info["shared"] == 300 and info["ordinary"] == 0
    check_against_oracle(jobs, results, 20, False)


def test_scale_launch_count_does_not_grow():
    big = mm.scale_jobs(5000)
    small = big[:200]
    b = many.Batch(False)
    r_small, i_small = many.align_many(small, 20, 2, batch=b, multi=True)
    r_big, i_big = many.align_many(big, 20, 2, batch=b, multi=True)
    print("info", i_small, i_big)
    assert i_big["shared"] == 5000 and i_big["ordinary"] == 0 and i_small["shared"] == 200
    assert i_big["launches"] == i_small["launches"] and i_big["launches"] > 0
    assert i_big["rounds"] == i_small["rounds"] == 1
    sample = sorted(random.Random(17).sample(range(5000), 200))
    check_against_oracle(big, r_big, 20, False, which=sample)
    check_against_oracle(small, r_small, 20, False, which=range(0, 200, 9))


def test_reuse_after_clear():
    """a batch of only multi-sequence jobs, then one of only pairs, then multi-sequence jobs again, through one Batch"""
    first = [seqs for _, _, seqs in mm.class_jobs(2, seed=5)]
    second = [list(pair) for _, pair in mc.class_jobs(2, seed=6)]
    b = many.Batch(False)
    r1, i1 = many.align_many(first, 20, 2, toupper=False, batch=b, multi=True)
    r2, i2 = many.align_many(second, 20, 2, toupper=False, batch=b)      # (multi=None: the batch keeps the switch)
    r3, i3 = many.align_many(first[::-1], 20, 2, toupper=False, batch=b)
    assert i1["shared"] == i1["jobs"] == len(first) and i2["shared"] == i2["jobs"] == len(second) and i3["shared"] == len(first)
    check_against_oracle(first, r1, 20, False)
    check_against_oracle(second, r2, 20, False)
    check_against_oracle(first[::-1], r3, 20, False)
