"""align_many with the reference's default picker on the device for pair jobs above 2048 ranks (reveal_amd/many.py `chain_large=`, csrc/rv_many.hip,
csrc/rv_pick_chain.hip, csrc/rv_leaf_chain.hip): every job's anchors and final text against `rem.align` of that job ALONE -- on the reference's own index
through tests/golden/many_chain_large.json, or the product's callback path run here -- never against align_many itself."""
import random

import pytest

import many_cases as mc
import many_chain_cases as cc
import many_chain_large_cases as cl
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jobs():
    return [list(pair) for _, pair in cl.jobs()]


@pytest.fixture(scope="module")
def golden():
    return cl.load_golden()


def got_of(r):
    return sorted((int(l), tuple(int(p) for p in pos)) for l, pos in r["anchors"]), cl.sha(r["T"])


def check_golden(results, want, what):
    bad = [(j, got_of(r)[0][:3], want[j][0][:3]) for j, r in enumerate(results) if got_of(r) != want[j]]
    assert not bad, "%s: %d jobs differ from rem.align on the reference's index, first: %r" % (what, len(bad), bad[:3])


def check_rem_align(jobs, results, kw, which):
    """against the product's own rem.align (Python callbacks on a stand-alone index of the job)"""
    bad = []
    for j in which:
        an, T = cc.rem_align_job(jobs[j], **kw)
        got, sha = got_of(results[j])
        if got != an or sha != cl.sha(T):
            bad.append((j, [len(s) for s in jobs[j]], got[:3], an[:3]))
    assert not bad, "%d jobs differ from rem.align, first: %r" % (len(bad), bad[:3])


CASES = [(n, False) for n, _ in cl.SETS] + [("default", True)]


@pytest.mark.parametrize("name,sa64", CASES)
def test_every_job_equals_the_reference_through_the_shared_launches(jobs, golden, name, sa64):
    kw = dict(cl.SETS)[name]
    results, info = many.align_many(jobs, minlength=kw["minlength"], sa64=sa64, picker=cl.picker_args(kw), chain_large=True)
    print("info", info)
    check_golden(results, golden[name], name)
    assert info["jobs"] == len(jobs) and info["shared"] == len(jobs) and info["ordinary"] == 0 and info["rounds"] == 1


@pytest.mark.parametrize("name,sa64", CASES)
def test_every_job_equals_the_reference_on_the_ordinary_path(jobs, golden, name, sa64):
    kw = dict(cl.SETS)[name]
    # (chain and large on: without the new switch neither takes a pair job above 2048 ranks under a picker)
    results, info = many.align_many(jobs, minlength=kw["minlength"], sa64=sa64, picker=cl.picker_args(kw), chain_large=False, chain=True, large=True)
    print("info", info)
    check_golden(results, golden[name], name)
    assert info["shared"] == 0 and info["ordinary"] == len(jobs)


@pytest.mark.parametrize("sa64", [False, True])
def test_positions_beyond_16_bits(golden, sa64):
    """the job of 80 002 ranks under its own set (a seedsize and a maxmums that admit it), with three small fillers so that the call reaches
    RV_MANY_CHAIN_LARGE_MIN.  Its TEXT positions go beyond 16 bits; the positions k_pick_chain packs, relative to the interval begins, stay below
    40 000 < 2^16 -- bit 16 of the packed fields is set by the jobs of 2^17 ranks of tests/test_gpu_many_chain_limits.py test_the_jobs_of_2_17_ranks"""
    name, kw = cl.BIG_SET
    batch = [list(cl.big_job())] + [list(p) for p in cl.fillers()]
    args = cl.picker_args(kw)
    assert all(many.takes_shared_launch([s.upper().encode() for s in j], picker=args, chain_large=True) for j in batch)
    results, info = many.align_many(batch, minlength=kw["minlength"], sa64=sa64, picker=args, chain_large=True)
    print("info", info)
    assert info["shared"] == 4 and info["ordinary"] == 0
    assert got_of(results[0]) == golden["big"][0]
    check_rem_align(batch, results, kw, [1, 2, 3])


def test_more_candidates_than_the_cap_flag_the_job(jobs, golden):
    """RV_PICK_CHAIN_CAP=8 (test hook): a sub-index with more than eight matches flags its job -- by condition (c) of the fixture some jobs hold more than
    64 at the root, others (identical, unrelated, homopolymer alleles) never more than a few; the flagged jobs finish on the ordinary path"""
    b = many.Batch()
    b.option("RV_PICK_CHAIN_CAP", 8)
    kw = dict(cl.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cl.picker_args(kw), chain_large=True, batch=b)
    print("info", info)
    assert 0 < info["shared"] < len(jobs) and info["shared"] + info["ordinary"] == len(jobs)
    assert info["ordinary"] >= sum(c > 8 for c in golden["candidates"][:-1])
    check_golden(results, golden["default"], "RV_PICK_CHAIN_CAP=8")


def test_a_level_without_device_tables_is_picked_by_the_host(jobs, golden):
    """RV_DECIDE_MAX_SUBS=0 (test hook): no level ships the tables of the device-side decisions, so every level's whole match list comes to the host and
    rv_pick_chain decides the sub-indices above 2048 ranks there -- never the longest match, which the fixture's rearranged jobs would show"""
    b = many.Batch()
    b.option("RV_DECIDE_MAX_SUBS", 0)
    kw = dict(cl.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cl.picker_args(kw), chain_large=True, batch=b)
    print("info", info)
    assert info["shared"] == len(jobs) and info["ordinary"] == 0
    check_golden(results, golden["default"], "RV_DECIDE_MAX_SUBS=0")


def test_a_flagged_job_of_a_large_round_finishes_on_the_ordinary_path(jobs, golden):
    """RV_MANY_CHAIN_FLAG=5 (test hook): every fifth job of the round counts as flagged; the results are the same"""
    b = many.Batch()
    b.option("RV_MANY_CHAIN_FLAG", 5)
    kw = dict(cl.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cl.picker_args(kw), chain_large=True, batch=b)
    flagged = (len(jobs) + 4) // 5
    assert info["shared"] == len(jobs) - flagged and info["ordinary"] == flagged and info["rounds"] == 1
    check_golden(results, golden["default"], "RV_MANY_CHAIN_FLAG=5")


def test_fewer_jobs_than_the_threshold_stay_ordinary(jobs, golden):
    kw = dict(cl.SETS)["default"]
    n = many.CHAIN_LARGE_MIN - 1
    sub = jobs[20:20 + n]
    results, info = many.align_many(sub, minlength=20, picker=cl.picker_args(kw), chain_large=True)
    assert info["shared"] == 0 and info["ordinary"] == n
    check_golden(results, golden["default"][20:20 + n], "below RV_MANY_CHAIN_LARGE_MIN")
    results, info = many.align_many(sub + [jobs[40]], minlength=20, picker=cl.picker_args(kw), chain_large=True)
    assert info["shared"] == n + 1 and info["ordinary"] == 0


def test_mixed_batch_with_every_switch_on(jobs, golden):
    """small pairs, large pairs (one with runs of N), a job of three sequences: info["shared"] is what takes_shared_launch says; a sample against the
    product's rem.align per job, the rest against the golden files"""
    kw = dict(minlength=20)
    args = cl.picker_args(kw)
    small = list(range(0, len(cc.jobs()), 9))
    large = list(range(0, len(jobs), 6))
    assert any(cl.jobs()[j][0] == "nruns" and "N" in jobs[j][0] for j in large)
    batch = [list(cc.jobs()[j][1]) for j in small] + [jobs[j] for j in large] + [mc.multi_jobs()[0]]
    want = [(cc.load_golden()["default"][j]) for j in small] + [golden["default"][j] for j in large] + [None]
    order = list(range(len(batch)))
    random.Random(12).shuffle(order)
    batch = [batch[k] for k in order]; want = [want[k] for k in order]
    results, info = many.align_many(batch, minlength=20, picker=args, chain=True, chain_multi=True, chain_wide=True, chain_large=True, multi=True, large=True,
                                    large_multi=True, wide=True)
    print("info", info)
    takes = [many.takes_shared_launch([s.upper().encode() for s in j], picker=args, chain=True, chain_multi=True, chain_wide=True, chain_large=True, minlength=20)
             for j in batch]
    assert all(takes) and info["shared"] == sum(takes) and info["ordinary"] == 0
    sample = set(random.Random(13).sample(range(len(batch)), 6)) | {k for k, w in enumerate(want) if w is None}
    check_rem_align(batch, results, kw, sorted(sample))
    for k, w in enumerate(want):
        if w is not None and k not in sample:
            assert got_of(results[k]) == w, k


def test_launches_do_not_depend_on_the_number_of_jobs(jobs, golden):
    sub = list(range(20, 32))
    b = many.Batch()
    kw = dict(cl.SETS)["default"]
    r1, i1 = many.align_many([jobs[j] for j in sub], minlength=20, picker=cl.picker_args(kw), chain_large=True, batch=b)
    r10, i10 = many.align_many([jobs[j] for j in sub] * 10, minlength=20, picker=cl.picker_args(kw), chain_large=True, batch=b)
    print("info", i1, i10)
    assert i1["shared"] == 12 and i10["shared"] == 120 and i1["rounds"] == i10["rounds"] == 1
    assert i1["launches"] == i10["launches"]
    check_golden(r1, [golden["default"][j] for j in sub], "once")
    check_golden(r10, [golden["default"][j] for j in sub] * 10, "ten times")


def test_several_rounds(jobs, golden):
    b = many.Batch()
    total = sum(len(a) + len(c) + 2 for a, c in jobs)
    b.option("RV_MANY_ROUND", total // 3)
    kw = dict(cl.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cl.picker_args(kw), chain_large=True, batch=b)
    print("info", info)
    assert info["shared"] == len(jobs) and info["ordinary"] == 0 and info["rounds"] >= 3
    check_golden(results, golden["default"], "three rounds")


def test_the_built_in_picker_is_back_after_a_picker_run(jobs, golden):
    """one Batch: a run with the picker and chain_large, then one without a picker and large=True -- the second equals the CPU oracle's built-in picker"""
    b = many.Batch()
    sub = list(range(18, 30))
    batch = [jobs[j] for j in sub]
    r1, i1 = many.align_many(batch, picker=cl.picker_args(dict(minlength=20)), chain_large=True, batch=b)
    r2, i2 = many.align_many(batch, large=True, batch=b)
    assert i1["shared"] == len(sub) and i2["shared"] == len(sub) and i1["ordinary"] == i2["ordinary"] == 0
    check_golden(r1, [golden["default"][j] for j in sub], "the picker's run")
    differ = 0
    for k, job in enumerate(batch):
        anchors, T = mc.oracle_job([s.upper().encode() for s in job], 20)
        got = sorted((int(l), tuple(int(p) for p in pos)) for l, pos in r2[k]["anchors"])
        assert got == anchors and r2[k]["T"].encode("latin-1") == T, k
        differ += got_of(r1[k])[0] != anchors
    assert differ >= 5          # (and the first run did use the other picker)
