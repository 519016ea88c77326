"""align_many with the reference's default picker on jobs of three and more sequences, on the device (reveal_amd/many.py `picker=`, `chain_multi=True`;
csrc/rv_many.hip, csrc/rv_leaf_multi_chain.hip): every job's anchors -- length and members in the order they are emitted -- and final text against
`rem.align` of that job ALONE: on the reference's own index through tests/golden/many_chain_multi.json, or the product's callback path run here; the
built-in picker against the CPU oracle.  Never against align_many itself."""
import random

import pytest

import many_cases as mc
import many_chain_cases as cc
import many_chain_multi_cases as cm
import many_multi_cases as mm
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jobs():
    return [list(seqs) for _, seqs in cm.jobs()]


@pytest.fixture(scope="module")
def golden():
    return cm.load_golden()


def as_bytes(job):
    return [s.encode() for s in job]


def got_of(r):
    return sorted((int(l), tuple(int(p) for p in pos)) for l, pos in r["anchors"]), cm.sha(r["T"])


def check_golden(results, want, what):
    bad = [(j, got_of(r)[0][:3], want[j][0][:3]) for j, r in enumerate(results) if got_of(r) != want[j]]
    assert not bad, "%s: %d jobs differ from rem.align on the reference's index, first: %r" % (what, len(bad), bad[:3])


def check_rem_align(jobs, results, kw, which=None):
    """against the product's own rem.align (Python callbacks on a stand-alone index of the job)"""
    bad = []
    for j in (range(len(jobs)) if which is None else which):
        an, T = cm.rem_align_job(jobs[j], **kw)
        got, sha = got_of(results[j])
        if got != an or sha != cm.sha(T):
            bad.append((j, [len(s) for s in jobs[j]], got[:3], an[:3]))
    assert not bad, "%d jobs differ from rem.align, first: %r" % (len(bad), bad[:3])


CASES = [(n, False) for n, _ in cm.SETS] + [("default", True)]


@pytest.mark.parametrize("name,sa64", CASES)
def test_every_job_equals_the_reference_through_the_shared_launch(jobs, golden, name, sa64):
    kw = dict(cm.SETS)[name]
    results, info = many.align_many(jobs, sa64=sa64, picker=cm.picker_args(kw), chain_multi=True, **cm.run_kw(kw))
    print("info", info)
    check_golden(results, golden[name], name)
    # (fixture condition (a): nothing raises in the reference, so nothing may be flagged)
    assert info["jobs"] == len(jobs) and info["shared"] == len(jobs) and info["ordinary"] == 0 and info["rounds"] == 1


@pytest.mark.parametrize("name,sa64", CASES)
def test_every_job_equals_the_reference_on_the_ordinary_path(jobs, golden, name, sa64):
    """the switch off: the fixture and the ordinary path agree"""
    kw = dict(cm.SETS)[name]
    results, info = many.align_many(jobs, sa64=sa64, picker=cm.picker_args(kw), chain=True, multi=True, chain_multi=False, **cm.run_kw(kw))
    print("info", info)
    check_golden(results, golden[name], name)
    assert info["shared"] == 0 and info["ordinary"] == len(jobs)


def mixed_batch():
    """pairs, a pair of 3000 ranks, jobs of 3 / 5 / 16 / 17 sequences, a job of 2049 ranks with k = 3"""
    rng = random.Random(19)
    out = [list(pair) for c, pair in cc.jobs() if c in ("rearranged", "indel")][::9]
    a = mc.rnd(rng, 1499)
    out.append([a, mc.mutate(rng, a, 0.01)])
    out += mc.multi_jobs()
    corners = {name: fam for name, fam, _ in mm.corner_jobs()}
    out += [corners["ranks_2049"], corners["k17"], mm.sized_job(rng, 16, 16 * 50), cm.rearranged(rng, 5), cm.rearranged(rng, 3)]
    rng.shuffle(out)
    return out


@pytest.mark.parametrize("kw", [dict(minlength=20), dict(minlength=20, seedsize=30), dict(minlength=20, trim=False), dict(minlength=0)],
                         ids=["default", "seedsize30", "notrim", "minl0"])
def test_mixed_batch_with_every_switch_on(kw):
    jobs = mixed_batch()
    args = cm.picker_args(kw)
    results, info = many.align_many(jobs, minlength=kw["minlength"], picker=args, chain=True, chain_multi=True, multi=True, large=True, large_multi=True, wide=True)
    print("info", info)
    want = [many.takes_shared_launch(as_bytes(j), picker=args, chain=True, chain_multi=True, minlength=kw["minlength"]) for j in jobs]
    plain = kw == dict(minlength=20)
    assert want == [plain and len(j) <= 16 and mm.ranks(j) <= 2048 for j in jobs]
    assert info["shared"] == sum(want) and info["ordinary"] == len(jobs) - sum(want)
    if plain:
        assert sum(w and len(j) >= 3 for w, j in zip(want, jobs)) >= 7 and 0 < info["shared"] < len(jobs)
    else:
        assert not any(w for w, j in zip(want, jobs) if len(j) >= 3)
    check_rem_align(jobs, results, kw)


def test_the_built_in_picker_is_back_after_a_picker_run(jobs):
    """one Batch: a run with the picker and the switch on, then one without a picker and multi=True -- the second equals the CPU oracle's built-in picker"""
    b = many.Batch()
    sub = jobs[5:45:2]
    r1, i1 = many.align_many(sub, picker=cm.picker_args(dict(minlength=20)), chain_multi=True, batch=b)
    r2, i2 = many.align_many(sub, multi=True, batch=b)
    assert i1["shared"] == len(sub) and i1["ordinary"] == 0 and i2["shared"] == len(sub) and i2["ordinary"] == 0
    differ = 0
    for j, job in enumerate(sub):
        anchors, T = mm.oracle_job([s.upper().encode() for s in job], 20)
        got = sorted((int(l), tuple(int(p) for p in pos)) for l, pos in r2[j]["anchors"])
        assert got == anchors and r2[j]["T"].encode("latin-1") == T, j
        differ += [(l, tuple(sorted(p))) for l, p in got_of(r1[j])[0]] != anchors
    assert differ >= 5          # (and the first run did use the other picker)


def test_several_rounds():
    jobs = mm.scale_jobs(300)
    b = many.Batch()
    b.option("RV_MANY_ROUND", 20000)
    kw = dict(minlength=20)
    results, info = many.align_many(jobs, picker=cm.picker_args(kw), chain_multi=True, batch=b)
    print("info", info)
    assert info["shared"] == 300 and info["ordinary"] == 0 and info["rounds"] > 2
    check_rem_align(jobs, results, kw, random.Random(2).sample(range(300), 40))


def test_launches_do_not_depend_on_the_number_of_jobs():
    big = mm.scale_jobs(20000)
    b = many.Batch()
    kw = dict(minlength=20)
    args = cm.picker_args(kw)
    r_small, i_small = many.align_many(big[:200], picker=args, chain_multi=True, batch=b)
    r_big, i_big = many.align_many(big, picker=args, chain_multi=True, batch=b)
    print("info", i_small, i_big)
    assert i_big["shared"] == 20000 and i_small["shared"] == 200 and i_big["ordinary"] == 0
    assert i_big["rounds"] == i_small["rounds"] == 1 and i_big["launches"] == i_small["launches"]
    check_rem_align(big, r_big, kw, random.Random(4).sample(range(20000), 100))


def test_anchors_straight_to_device_memory(jobs, golden):
    """RV_LEAF_ACAP=2: a workgroup stages two anchors and writes the others one by one"""
    b = many.Batch()
    b.option("RV_LEAF_ACAP", 2)
    kw = dict(cm.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cm.picker_args(kw), chain_multi=True, batch=b)
    assert info["shared"] == len(jobs)
    assert max(len(r["anchors"]) for r in results) > 2
    check_golden(results, golden["default"], "RV_LEAF_ACAP=2")


def test_a_flagged_job_finishes_on_the_ordinary_path(jobs, golden):
    """RV_MANY_CHAIN_FLAG=5 (test hook): every fifth job of the round counts as flagged by the kernel -- where the reference's trim_overlap would raise -- so its
    anchors are dropped and it runs the ordinary way with the host picker; the results are the same"""
    b = many.Batch()
    b.option("RV_MANY_CHAIN_FLAG", 5)
    kw = dict(cm.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cm.picker_args(kw), chain_multi=True, batch=b)
    flagged = (len(jobs) + 4) // 5
    assert info["shared"] == len(jobs) - flagged and info["ordinary"] == flagged and info["rounds"] == 1
    check_golden(results, golden["default"], "RV_MANY_CHAIN_FLAG=5")
