"""align_many with RV_MANY_WIDE on the device (reveal_amd/many.py, csrc/rv_many.hip, csrc/rv_leaf_multi.hip, csrc/rv_many_large.hip): jobs of
17 .. 64 sequences through the shared launches.  Every job's anchors, final text and (RV_MANY_KEEP) SA / LCP are checked against the CPU oracle
run on that job ALONE (many_multi_cases.oracle_job: assemble + construct + align_bench) -- never against the ordinary path or align_many
itself.  tests/test_cpu_many_wide.py shows from the oracle alone that these jobs have anchors."""
import random

import numpy as np
import pytest

import many_cases as mc
import many_large_multi_cases as lm
import many_multi_cases as mm
import many_wide_cases as mw
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

pytestmark = pytest.mark.gpu

MINL = 12      # members of a job of 64 sequences and 2048 ranks are 31 bases long: at minlength 20 few of those jobs have an anchor


def as_bytes(job):
    return [s.encode() if isinstance(s, str) else s for s in job]


def ranks(job):
    return sum(len(s) for s in job) + len(job)


def is_wide(job):
    return many.MULTI_KMAX < len(job) <= many.WIDE_KMAX


def is_wide_large(job, large_max=many.LARGE_MAX):
    return is_wide(job) and many.LEAF_RANKS < ranks(job) <= large_max


def shared_with(jobs, wide_large_min, **switches):
    """takes_shared_launch per job, and the rule of the call on top of it: fewer jobs of 17 .. 64 sequences above 2048 ranks than
    RV_MANY_WIDE_LARGE_MIN stay ordinary"""
    want = [many.takes_shared_launch(as_bytes(j), **switches) for j in jobs]
    nlarge = sum(1 for j, w in zip(jobs, want) if w and is_wide_large(j))
    if nlarge < wide_large_min:
        want = [w and not is_wide_large(j) for j, w in zip(jobs, want)]
    return want


def check_against_oracle(jobs, results, minl, sa64, minn=2, which=None):
    bad = []
    total_l = nanch = 0
    for j in (range(len(jobs)) if which is None else which):
        anchors, T = mm.oracle_job(jobs[j], minl, minn, sa64)
        got = sorted((int(l), tuple(int(p) for p in pos)) for l, pos in results[j]["anchors"])
        if got != anchors or results[j]["T"].encode("latin-1") != T:
            bad.append((j, len(jobs[j]), ranks(jobs[j]), got[:2], anchors[:2]))
        total_l += sum(l for l, _ in anchors)
        nanch += len(anchors)
    assert not bad, "%d jobs differ from the oracle, first: %r" % (len(bad), bad[:2])
    return nanch, total_l


def check_arrays(b, jobs, which, sa64):
    bad = []
    for j in which:
        _, _, sa, lcp = mm.oracle_job(jobs[j], 20, 2, sa64, arrays=True)
        gsa, glcp = b.arrays(j)
        if not (np.array_equal(gsa, sa) and np.array_equal(glcp.astype(np.int64), lcp.astype(np.int64))):
            bad.append((j, len(jobs[j]), ranks(jobs[j]), int(np.argmax(gsa != sa)) if not np.array_equal(gsa, sa) else -1))
    assert not bad, "%d jobs' arrays differ, first: %r" % (len(bad), bad[:5])


def main_batch():
    """20 class jobs for every k of 17 .. 64 (120), the corner jobs, 11 pair jobs, 9 jobs of 3 .. 16 sequences, shuffled"""
    jobs = [seqs for _, _, seqs in mw.class_jobs(20)]
    jobs += [seqs for _, seqs, _ in mw.corner_jobs()]
    jobs += [list(pair) for _, pair in mc.class_jobs(1)]
    jobs += [seqs for _, _, seqs in mm.class_jobs(1)]
    random.Random(2).shuffle(jobs)
    return jobs


@pytest.mark.parametrize("sa64", [False, True])
def test_every_job_equals_the_oracle_in_one_call(sa64):
    jobs = main_batch()
    results, info = many.align_many(jobs, minlength=MINL, minn=2, sa64=sa64, toupper=False, wide=True)
    print("info", info)
    want = shared_with(jobs, many.WIDE_LARGE_MIN, wide=True)
    wide = [j for j in range(len(jobs)) if is_wide(jobs[j])]
    assert len(wide) == 120 + 5 and {len(jobs[j]) for j in wide} == set(mw.K_VALUES)
    assert sum(1 for j in wide if want[j]) == 120 + 4             # all but the one job of 2049 ranks: fewer of its class than the threshold
    assert not any(want[j] for j in range(len(jobs)) if len(jobs[j]) > 64 or 3 <= len(jobs[j]) <= 16)
    assert info["jobs"] == len(jobs) == len(results)
    assert info["shared"] == sum(want) and info["ordinary"] == len(jobs) - sum(want)      # no eligible job fell back, none was dropped
    nanch, total_l = check_against_oracle(jobs, results, MINL, sa64)
    assert sum(1 for j in wide if results[j]["anchors"]) > len(wide) // 2
    assert any(len(pos) == 64 for j in wide for _, pos in results[j]["anchors"])          # a full ballot
    assert any(len(pos) < len(jobs[j]) for j in wide for _, pos in results[j]["anchors"])
    assert info["stats"]["splits"] == nanch and info["stats"]["anchored_bp"] == total_l


def test_results_do_not_depend_on_the_switch():
    jobs = main_batch()
    results, info = many.align_many(jobs, minlength=MINL, minn=2, toupper=False, wide=False)
    want = shared_with(jobs, many.WIDE_LARGE_MIN, wide=False)
    assert info["shared"] == sum(want) == sum(1 for j in jobs if len(j) == 2 and ranks(j) <= 2048)
    assert info["ordinary"] == len(jobs) - sum(want)              # every wide job among them
    check_against_oracle(jobs, results, MINL, False)
    r_none, i_none = many.align_many(jobs, minlength=MINL, minn=2, toupper=False)      # off unless asked for
    assert (i_none["shared"], i_none["ordinary"], i_none["rounds"], i_none["launches"]) == (info["shared"], info["ordinary"], info["rounds"], info["launches"])


@pytest.mark.parametrize("sa64", [False, True])
def test_arrays_equal_the_stand_alone_construct(sa64):
    """RV_MANY_KEEP: SA and LCP of every shared wide job = construct() of that job alone; identical members and duplicates: up to 64 suffixes
    tie through '$' at every position and have to come out in the stand-alone order"""
    rng = random.Random(44)
    jobs = [seqs for _, _, seqs in mw.class_jobs(6, seed=45, classes=("identical", "sites"), k_values=(17, 33, 64))]
    for k in (17, 33, 64):                                        # duplicates: two alleles, each in about half of the members
        a, b = mc.rnd(rng, mw.top_length(k)), mc.rnd(rng, mw.top_length(k) - 1)
        jobs.append([a if rng.random() < 0.5 else b for _ in range(k)])
    jobs += [seqs for _, seqs, kind in mw.corner_jobs() if kind == "small"]
    b = many.Batch(sa64)
    b.option("RV_MANY_KEEP", 1)
    b.option("RV_MANY_WIDE", 1)
    for j in jobs:
        b.add(as_bytes(j))
    b.run(20, 2)
    assert b.info()["shared"] == len(jobs) and b.info()["ordinary"] == 0
    check_arrays(b, jobs, range(len(jobs)), sa64)


def test_minn():
    """minn 2, 3, k and k + 1 at k = 33 and k = 64: a sub-index of fewer than minn samples anchors nothing; k + 1: nothing at all"""
    fams = mw.class_jobs(12, seed=77, classes=("dropout", "sites"), k_values=(33, 64))
    for sel in ("2", "3", "k", "k+1"):
        groups = {}
        for _, k, seqs in fams:
            groups.setdefault({"2": 2, "3": 3, "k": k, "k+1": k + 1}[sel], []).append(seqs)
        for minn, jobs in sorted(groups.items()):
            results, info = many.align_many(jobs, MINL, minn, toupper=False, wide=True)
            assert info["shared"] == len(jobs)
            nanch, _ = check_against_oracle(jobs, results, MINL, False, minn=minn)
            if sel == "k+1":
                assert nanch == 0
            else:
                assert nanch > 0


@pytest.mark.parametrize("minl", [1, 5])
@pytest.mark.parametrize("stage", [256, 2])
def test_minlength_and_the_direct_anchor_path(minl, stage):
    """minlength 1 and 5 on jobs of at most 600 ranks; RV_MANY_STAGE 2: all but two anchors of a job (of up to 64 members each) leave the
    workgroup directly, not through its staging"""
    jobs = mw.short_jobs(12)
    b = many.Batch(False)
    b.option("RV_MANY_STAGE", stage)
    results, info = many.align_many(jobs, minl, 2, toupper=False, batch=b, wide=True)
    assert info["shared"] == len(jobs) and info["ordinary"] == 0
    nanch, total_l = check_against_oracle(jobs, results, minl, False)
    assert info["stats"]["splits"] == nanch and info["stats"]["anchored_bp"] == total_l
    if minl == 1:
        assert max(len(r["anchors"]) for r in results) > 2


def test_rounds_and_scale():
    """rounds split the jobs; the launches of a call do not grow with its jobs"""
    big = mw.scale_jobs(2000)
    small = big[:200]
    b = many.Batch(False)
    r_small, i_small = many.align_many(small, MINL, 2, toupper=False, batch=b, wide=True)
    r_big, i_big = many.align_many(big, MINL, 2, toupper=False, batch=b, wide=True)
    print("info", i_small, i_big)
    assert i_big["shared"] == 2000 and i_big["ordinary"] == 0 and i_small["shared"] == 200
    assert i_big["launches"] == i_small["launches"] and i_big["launches"] > 0
    assert i_big["rounds"] == i_small["rounds"] == 1
    check_against_oracle(big, r_big, MINL, False, which=sorted(random.Random(17).sample(range(2000), 150)))
    check_against_oracle(small, r_small, MINL, False, which=range(0, 200, 9))
    b.option("RV_MANY_ROUND", 60000)
    r_split, i_split = many.align_many(small, MINL, 2, toupper=False, batch=b)
    assert i_split["rounds"] > 3 and i_split["shared"] == 200 and i_split["ordinary"] == 0
    check_against_oracle(small, r_split, MINL, False)


def test_large_wide_jobs():
    """jobs of 17, 33 and 64 sequences of 2049 .. 6000 ranks: shared from RV_MANY_WIDE_LARGE_MIN such jobs on, ordinary below; the arrays"""
    jobs = [seqs for _, _, seqs in mw.large_jobs(8)] + [seqs for _, seqs, kind in mw.corner_jobs() if kind == "large"]
    assert len(jobs) == 25 and all(is_wide_large(j) for j in jobs) and {len(j) for j in jobs} == {17, 33, 64}
    b = many.Batch(False)
    b.option("RV_MANY_WIDE_LARGE_MIN", 1)
    b.option("RV_MANY_KEEP", 1)
    results, info = many.align_many(jobs, MINL, 2, toupper=False, batch=b, wide=True)
    print("info", info)
    assert info["shared"] == len(jobs) and info["ordinary"] == 0 and info["rounds"] == 1
    nanch, total_l = check_against_oracle(jobs, results, MINL, False)
    assert info["stats"]["splits"] == nanch and info["stats"]["anchored_bp"] == total_l and nanch > len(jobs)
    check_arrays(b, jobs, range(len(jobs)), False)
    # the default threshold, fewer jobs than it: counted ordinary, the same results
    few = jobs[:many.WIDE_LARGE_MIN - 1]
    results, info = many.align_many(few, MINL, 2, toupper=False, wide=True)
    assert info["shared"] == 0 and info["ordinary"] == len(few) and info["rounds"] == 0
    check_against_oracle(few, results, MINL, False)
    # ... and as many as it: shared
    results, info = many.align_many(jobs[:many.WIDE_LARGE_MIN], MINL, 2, toupper=False, wide=True)
    assert info["shared"] == many.WIDE_LARGE_MIN and info["ordinary"] == 0


def every_switch_jobs():
    """wide jobs on both sides of 2048 ranks among jobs of 3 .. 16 sequences above 2048 ranks, small ones and pairs, and a job of 65 sequences, shuffled"""
    wide_large = [seqs for _, _, seqs in mw.large_jobs(2, seed=13)]
    jobs = wide_large + lm.sized_jobs(5, seed=18) + [seqs for _, seqs, _ in mw.corner_jobs()] + mm.small_jobs(4, seed=19)
    jobs += [list(p) for _, p in mc.class_jobs(1, seed=20)][:5] + [list(p) for p in mc.big_pairs(2, seed=21)]
    random.Random(5).shuffle(jobs)
    return jobs


def test_every_switch_on():
    """one call with all four switches on: the jobs of every_switch_jobs -- every class in rounds of its own, nothing ordinary but the job of 65 sequences"""
    jobs = every_switch_jobs()
    b = many.Batch(False)
    for name, v in (("RV_MANY_WIDE_LARGE_MIN", 1), ("RV_MANY_LARGE_MULTI_MIN", 1), ("RV_MANY_LARGE_MIN", 1)):
        b.option(name, v)
    results, info = many.align_many(jobs, MINL, 2, toupper=False, batch=b, multi=True, large=True, large_multi=True, wide=True)
    print("info", info)
    want = shared_with(jobs, 1, multi=True, large=True, large_multi=True, wide=True)
    assert sum(want) == len(jobs) - 1 and [len(j) for j, w in zip(jobs, want) if not w] == [65]
    assert info["shared"] == sum(want) and info["ordinary"] == 1
    assert info["rounds"] == 6                                    # pairs, large pairs, 3 .. 16 small, 3 .. 16 large, wide small, wide large
    check_against_oracle(jobs, results, MINL, False)
    # without the wide switch the same batch leaves exactly the wide jobs ordinary, and its other rounds are what they were
    r_off, i_off = many.align_many(jobs, MINL, 2, toupper=False, batch=b, wide=False)
    nwide = sum(1 for j in jobs if is_wide(j))
    assert nwide == 6 + 5 and i_off["ordinary"] == 1 + nwide and i_off["shared"] == len(jobs) - 1 - nwide and i_off["rounds"] == 4
    check_against_oracle(jobs, r_off, MINL, False)


def test_reuse_after_clear():
    """a batch of only wide jobs, then one of only pairs, then wide jobs again, through one Batch"""
    first = [seqs for _, _, seqs in mw.class_jobs(3, seed=5)]
    second = [list(pair) for _, pair in mc.class_jobs(2, seed=6)]
    b = many.Batch(False)
    r1, i1 = many.align_many(first, MINL, 2, toupper=False, batch=b, wide=True)
    r2, i2 = many.align_many(second, MINL, 2, toupper=False, batch=b)      # (wide=None: the batch keeps the switch)
    r3, i3 = many.align_many(first[::-1], MINL, 2, toupper=False, batch=b)
    assert i1["shared"] == i1["jobs"] == len(first) and i2["shared"] == i2["jobs"] == len(second) and i3["shared"] == len(first)
    check_against_oracle(first, r1, MINL, False)
    check_against_oracle(second, r2, MINL, False)
    check_against_oracle(first[::-1], r3, MINL, False)


def test_argument_errors():
    b = many.Batch(False)
    with pytest.raises(many.error):
        b.option("RV_MANY_WIDE_LARGE_MIN", -1)
    b.option("RV_MANY_WIDE", 0)
    b.option("RV_MANY_WIDE_LARGE_MIN", 0)
