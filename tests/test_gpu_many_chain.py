"""align_many with the reference's default picker on the device (reveal_amd/many.py `picker=`, csrc/rv_many.hip, csrc/rv_leaf_chain.hip): every job's
anchors and final text against `rem.align` of that job ALONE -- on the reference's own index through tests/golden/many_chain.json, or the product's
callback path run here -- never against align_many itself."""
import random

import pytest

import many_cases as mc
import many_chain_cases as cc
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many, schemes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jobs():
    return [list(pair) for _, pair in cc.jobs()]


@pytest.fixture(scope="module")
def golden():
    return cc.load_golden()


def got_of(r):
    return sorted((int(l), tuple(int(p) for p in pos)) for l, pos in r["anchors"]), cc.sha(r["T"])


def check_golden(results, want, what):
    bad = [(j, got_of(r)[0][:3], want[j][0][:3]) for j, r in enumerate(results) if got_of(r) != want[j]]
    assert not bad, "%s: %d jobs differ from rem.align on the reference's index, first: %r" % (what, len(bad), bad[:3])


def check_rem_align(jobs, results, kw, which=None):
    """against the product's own rem.align (Python callbacks on a stand-alone index of the job)"""
    bad = []
    for j in (range(len(jobs)) if which is None else which):
        an, T = cc.rem_align_job(jobs[j], **kw)
        got, sha = got_of(results[j])
        if got != an or sha != cc.sha(T):
            bad.append((j, [len(s) for s in jobs[j]], got[:3], an[:3]))
    assert not bad, "%d jobs differ from rem.align, first: %r" % (len(bad), bad[:3])


CASES = [(n, False) for n, _ in cc.SETS] + [("default", True)]


@pytest.mark.parametrize("name,sa64", CASES)
def test_every_job_equals_the_reference_through_the_shared_launch(jobs, golden, name, sa64):
    kw = dict(cc.SETS)[name]
    results, info = many.align_many(jobs, minlength=kw["minlength"], sa64=sa64, picker=cc.picker_args(kw), chain=True)
    print("info", info)
    check_golden(results, golden[name], name)
    assert info["jobs"] == len(jobs) and info["shared"] == len(jobs) and info["ordinary"] == 0 and info["rounds"] == 1


@pytest.mark.parametrize("name,sa64", CASES)
def test_every_job_equals_the_reference_on_the_ordinary_path(jobs, golden, name, sa64):
    kw = dict(cc.SETS)[name]
    results, info = many.align_many(jobs, minlength=kw["minlength"], sa64=sa64, picker=cc.picker_args(kw), chain=False)
    print("info", info)
    check_golden(results, golden[name], name)
    assert info["shared"] == 0 and info["ordinary"] == len(jobs)


def mixed_batch():
    """admitted pairs, a pair of 3000 ranks, jobs of three and five sequences"""
    rng = random.Random(9)
    out = [list(pair) for c, pair in cc.jobs() if c in ("rearranged", "indel", "tandem")][::7]
    a = mc.rnd(rng, 1499)
    out.append([a, mc.mutate(rng, a, 0.01)])
    out += mc.multi_jobs()
    rng.shuffle(out)
    return out


@pytest.mark.parametrize("kw", [dict(minlength=20), dict(minlength=20, seedsize=30), dict(minlength=20, trim=False), dict(minlength=0)],
                         ids=["default", "seedsize30", "notrim", "minl0"])
def test_mixed_batch_with_every_switch_on(kw):
    jobs = mixed_batch()
    if len(kw) > 1 or kw["minlength"] == 0:
        jobs = jobs[::2]          # (the calls nothing of which is admitted: every job twice through a level loop, here and in rem.align)
    args = cc.picker_args(kw)
    results, info = many.align_many(jobs, minlength=kw["minlength"], picker=args, chain=True, multi=True, large=True, large_multi=True, wide=True)
    print("info", info)
    want = [many.takes_shared_launch([s.encode() for s in j], picker=args, chain=True, minlength=kw["minlength"]) for j in jobs]
    assert want == [len(j) == 2 and sum(map(len, j)) + 2 <= 2048 and kw == dict(minlength=20) for j in jobs]
    assert info["shared"] == sum(want) and info["ordinary"] == len(jobs) - sum(want)
    if kw == dict(minlength=20):
        assert 0 < info["shared"] < len(jobs)
    check_rem_align(jobs, results, kw)


def test_the_built_in_picker_is_back_after_a_picker_run(jobs):
    """one Batch: a run with the picker, then one without -- the second equals the CPU oracle's built-in picker, nothing leaked"""
    b = many.Batch()
    sub = jobs[cc.N_CLASS:cc.N_CLASS + 30] + [list(p) for p in mc.big_pairs(2)]
    r1, i1 = many.align_many(sub, picker=schemes.PickerArgs(maxmums=10000), chain=True, batch=b)
    r2, i2 = many.align_many(sub, batch=b)
    assert i1["shared"] == 30 and i1["ordinary"] == 2 and i2["shared"] == 30 and i2["ordinary"] == 2
    differ = 0
    for j, job in enumerate(sub):
        anchors, T = mc.oracle_job([s.upper().encode() for s in job], 20)
        got = sorted((int(l), tuple(int(p) for p in pos)) for l, pos in r2[j]["anchors"])
        assert got == anchors and r2[j]["T"].encode("latin-1") == T, j
        differ += got_of(r1[j])[0] != anchors
    assert differ >= 10          # (and the first run did use the other picker)


def test_several_rounds():
    jobs = [list(p) for p in mc.scale_jobs(300)]
    b = many.Batch()
    b.option("RV_MANY_ROUND", 20000)
    kw = dict(minlength=20)
    results, info = many.align_many(jobs, picker=cc.picker_args(kw), chain=True, batch=b)
    print("info", info)
    assert info["shared"] == 300 and info["ordinary"] == 0 and info["rounds"] > 2
    check_rem_align(jobs, results, kw, random.Random(2).sample(range(300), 40))


def test_launches_do_not_depend_on_the_number_of_jobs():
    big = [list(p) for p in mc.scale_jobs(20000)]
    b = many.Batch()
    kw = dict(minlength=20)
    args = cc.picker_args(kw)
    r_small, i_small = many.align_many(big[:200], picker=args, chain=True, batch=b)
    r_big, i_big = many.align_many(big, picker=args, chain=True, batch=b)
    print("info", i_small, i_big)
    assert i_big["shared"] == 20000 and i_small["shared"] == 200 and i_big["ordinary"] == 0
    assert i_big["rounds"] == i_small["rounds"] == 1 and i_big["launches"] == i_small["launches"]
    check_rem_align(big, r_big, kw, random.Random(4).sample(range(20000), 100))


def test_anchors_straight_to_device_memory(jobs, golden):
    """RV_LEAF_ACAP=2: a workgroup stages two anchors and writes the others one by one"""
    b = many.Batch()
    b.option("RV_LEAF_ACAP", 2)
    kw = dict(cc.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cc.picker_args(kw), chain=True, batch=b)
    assert info["shared"] == len(jobs)
    assert max(len(r["anchors"]) for r in results) > 2
    check_golden(results, golden["default"], "RV_LEAF_ACAP=2")


def test_a_flagged_job_finishes_on_the_ordinary_path(jobs, golden):
    """RV_MANY_CHAIN_FLAG=5 (test hook): every fifth job of the round counts as flagged by the kernel -- where the reference's trim_overlap would raise -- so its
    anchors are dropped and it runs the ordinary way with the host picker; the results are the same"""
    b = many.Batch()
    b.option("RV_MANY_CHAIN_FLAG", 5)
    kw = dict(cc.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cc.picker_args(kw), chain=True, batch=b)
    flagged = (len(jobs) + 4) // 5
    assert info["shared"] == len(jobs) - flagged and info["ordinary"] == flagged and info["rounds"] == 1
    check_golden(results, golden["default"], "RV_MANY_CHAIN_FLAG=5")


def test_set_picker_refuses_what_it_does_not_know():
    b = many.Batch()
    A = many.picker_struct(schemes.PickerArgs())
    import ctypes
    assert b._dll.rv_many_set_picker(b._m, 1, None) == -1 and "options" in b._lib.err()
    assert b._dll.rv_many_set_picker(b._m, 2, ctypes.byref(A)) == -1 and "kind" in b._lib.err()
    A.gcmodel = 7
    assert b._dll.rv_many_set_picker(b._m, 1, ctypes.byref(A)) == -1 and "gap cost model" in b._lib.err()
    assert b._dll.rv_many_set_picker(b._m, 0, None) == 0
