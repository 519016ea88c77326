"""align_many with the reference's default picker on jobs of 17 .. 64 sequences, on the device (reveal_amd/many.py `picker=`, `chain_wide=True`;
csrc/rv_many.hip, the 64-sample form of k_leaf_multi_chain in csrc/rv_leaf_multi_chain.hip): every job's anchors -- length and members in the order they
are emitted -- and final text against `rem.align` of that job ALONE: on the reference's own index through tests/golden/many_chain_wide.json, or the
product's callback path run here; the built-in picker against the CPU oracle.  Never against align_many itself."""
import random

import pytest

import many_cases as mc
import many_chain_cases as cc
import many_chain_multi_cases as cm
import many_chain_wide_cases as cw
import many_multi_cases as mm
import many_wide_cases as mw
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jobs():
    return [list(seqs) for _, seqs in cw.jobs()]


@pytest.fixture(scope="module")
def golden():
    return cw.load_golden()


def as_bytes(job):
    return [s.encode() for s in job]


def got_of(r):
    return sorted((int(l), tuple(int(p) for p in pos)) for l, pos in r["anchors"]), cw.sha(r["T"])


def check_golden(results, want, what):
    bad = [(j, got_of(r)[0][:2], want[j].get("anchors", want[j])[:2]) for j, r in enumerate(results) if not cw.same(want[j], *got_of(r))]
    assert not bad, "%s: %d jobs differ from rem.align on the reference's index, first: %r" % (what, len(bad), bad[:2])


def check_rem_align(jobs, results, kw, which=None):
    """against the product's own rem.align (Python callbacks on a stand-alone index of the job)"""
    bad = []
    for j in (range(len(jobs)) if which is None else which):
        an, T = cw.rem_align_job(jobs[j], **kw)
        got, sha = got_of(results[j])
        if got != an or sha != cw.sha(T):
            bad.append((j, len(jobs[j]), mm.ranks(jobs[j]), got[:2], an[:2]))
    assert not bad, "%d jobs differ from rem.align, first: %r" % (len(bad), bad[:2])


CASES = [(n, False) for n, _ in cw.SETS] + [("default", True)]


@pytest.mark.parametrize("name,sa64", CASES)
def test_every_job_equals_the_reference_through_the_shared_launch(jobs, golden, name, sa64):
    kw = dict(cw.SETS)[name]
    results, info = many.align_many(jobs, sa64=sa64, picker=cw.picker_args(kw), chain_wide=True, **cw.run_kw(kw))
    print("info", info)
    check_golden(results, golden[name], name)
    # (nothing raises in the reference, and the job list was chosen so that the pick stage never gives up: nothing may be flagged)
    assert info["jobs"] == len(jobs) and info["shared"] == len(jobs) and info["ordinary"] == 0 and info["rounds"] == 1


@pytest.mark.parametrize("name,sa64", CASES)
def test_every_job_equals_the_reference_on_the_ordinary_path(jobs, golden, name, sa64):
    """the switch off: the fixture and the ordinary path agree"""
    kw = dict(cw.SETS)[name]
    results, info = many.align_many(jobs, sa64=sa64, picker=cw.picker_args(kw), chain=True, chain_multi=True, multi=True, wide=True, chain_wide=False, **cw.run_kw(kw))
    print("info", info)
    check_golden(results, golden[name], name)
    assert info["shared"] == 0 and info["ordinary"] == len(jobs)


def mixed_batch():
    """pairs, a pair of 3000 ranks, jobs of 3 / 5 / 16 sequences, jobs of 17 / 24 / 33 / 64 sequences, a job of 64 sequences and 2049 ranks, a job of 65;
    every job of at most 64 sequences has a member of 30 bases or more, so that seedsize=30 can reach all of them"""
    rng = random.Random(23)
    out = [list(pair) for c, pair in cc.jobs() if c in ("rearranged", "indel")][::12]
    a = mc.rnd(rng, 1499)
    out.append([a, mc.mutate(rng, a, 0.01)])
    out += [cm.rearranged(rng, 3), cm.rearranged(rng, 5), mm.sized_job(rng, 16, 16 * 50)]
    wide = {name: fam for name, fam, _ in mw.corner_jobs()}
    out += [cw.shuffled(rng, 17), cw.shuffled(rng, 33), cw.shuffled(rng, 24), mw.make_family("sites", rng, 33), wide["k64_full"], wide["k17"]]
    out += [wide["k64_2049"], wide["k65"]]
    rng.shuffle(out)
    return out


@pytest.mark.parametrize("kw", [dict(minlength=20), dict(minlength=5), dict(minlength=20, seedsize=30), dict(minlength=20, trim=False), dict(minlength=0)],
                         ids=["default", "minl5", "seedsize30", "notrim", "minl0"])
def test_mixed_batch_with_every_switch_on(kw):
    jobs = mixed_batch()
    assert sorted({len(j) for j in jobs}) == [2, 3, 5, 16, 17, 24, 33, 64, 65] and min(max(len(s) for s in j) for j in jobs if len(j) <= 64) >= 30 and max(mm.ranks(j) for j in jobs if len(j) == 2) == 3000
    args = cw.picker_args(kw)
    results, info = many.align_many(jobs, minlength=kw["minlength"], picker=args, chain=True, chain_multi=True, chain_wide=True, multi=True, large=True,
                                    large_multi=True, wide=True)
    print("info", info)
    want = [many.takes_shared_launch(as_bytes(j), picker=args, chain=True, chain_multi=True, chain_wide=True, minlength=kw["minlength"]) for j in jobs]
    plain = "seedsize" not in kw and "trim" not in kw and kw["minlength"] > 0
    assert want == [plain and len(j) <= 64 and mm.ranks(j) <= 2048 for j in jobs]
    assert info["shared"] == sum(want) and info["ordinary"] == len(jobs) - sum(want)
    if plain:
        assert sum(w and len(j) >= 17 for w, j in zip(want, jobs)) == 6 and 0 < info["shared"] < len(jobs)
    else:
        assert not any(w for w, j in zip(want, jobs) if len(j) >= 17)      # no wide job is shared
    check_rem_align(jobs, results, kw)


def test_the_built_in_picker_is_back_after_a_picker_run(jobs):
    """one Batch: a run with the picker and the switch on, then one without a picker and wide=True -- the second equals the CPU oracle's built-in picker"""
    b = many.Batch()
    sub = jobs[1::3]
    r1, i1 = many.align_many(sub, picker=cw.picker_args(dict(minlength=20)), chain_wide=True, batch=b)
    r2, i2 = many.align_many(sub, wide=True, batch=b)
    assert i1["shared"] == len(sub) and i1["ordinary"] == 0 and i2["shared"] == len(sub) and i2["ordinary"] == 0
    differ = 0
    for j, job in enumerate(sub):
        anchors, T = mm.oracle_job([s.upper().encode() for s in job], 20)
        got = sorted((int(l), tuple(int(p) for p in pos)) for l, pos in r2[j]["anchors"])
        assert got == anchors and r2[j]["T"].encode("latin-1") == T, j
        differ += [(l, tuple(sorted(p))) for l, p in got_of(r1[j])[0]] != anchors
    assert differ >= 5          # (and the first run did use the other picker)


def test_several_rounds():
    jobs = mw.scale_jobs(300)
    b = many.Batch()
    b.option("RV_MANY_ROUND", 100000)
    kw = dict(minlength=20)
    results, info = many.align_many(jobs, picker=cw.picker_args(kw), chain_wide=True, batch=b)
    print("info", info)
    assert info["shared"] == 300 and info["ordinary"] == 0 and info["rounds"] > 2
    check_rem_align(jobs, results, kw, random.Random(2).sample(range(300), 40))


def test_launches_do_not_depend_on_the_number_of_jobs():
    big = mw.scale_jobs(2000)
    b = many.Batch()
    kw = dict(minlength=20)
    args = cw.picker_args(kw)
    r_small, i_small = many.align_many(big[:200], picker=args, chain_wide=True, batch=b)
    r_big, i_big = many.align_many(big, picker=args, chain_wide=True, batch=b)
    print("info", i_small, i_big)
    assert i_big["shared"] == 2000 and i_small["shared"] == 200 and i_big["ordinary"] == 0 and i_small["ordinary"] == 0
    assert i_big["rounds"] == i_small["rounds"] == 1 and i_big["launches"] == i_small["launches"]
    check_rem_align(big, r_big, kw, random.Random(4).sample(range(2000), 20))


def test_anchors_straight_to_device_memory(jobs, golden):
    """RV_LEAF_ACAP=2: a workgroup stages two anchors and writes the others one by one"""
    b = many.Batch()
    b.option("RV_LEAF_ACAP", 2)
    kw = dict(cw.SETS)["minl5"]
    results, info = many.align_many(jobs, picker=cw.picker_args(kw), chain_wide=True, batch=b, **cw.run_kw(kw))
    assert info["shared"] == len(jobs)
    assert max(len(r["anchors"]) for r in results) > 2
    check_golden(results, golden["minl5"], "RV_LEAF_ACAP=2")


def test_the_job_the_kernel_flags_by_itself():
    """many_chain_wide_cases.flagged_job() at minlength 1: a sub-index holds two matches with the split's offsets, the kernel's own twin check fires (flag 8,
    no test hook), the job is dropped from the round and finishes on the ordinary path -- the result is rem.align's, among neighbours that stay shared"""
    rng = random.Random(31)
    batch = [cw.shuffled(rng, 17), cw.flagged_job(), cw.shuffled(rng, 33)]
    kw = dict(minlength=1)
    results, info = many.align_many(batch, minlength=1, picker=cw.picker_args(kw), chain_wide=True)
    print("info", info)
    assert info["jobs"] == 3 and info["ordinary"] == 1 and info["shared"] == 2 and info["rounds"] == 1
    check_rem_align(batch, results, kw)
    # with the switch off the same results
    results0, info0 = many.align_many(batch, minlength=1, picker=cw.picker_args(kw), chain_wide=False)
    assert info0["ordinary"] == 3 and [got_of(r) for r in results0] == [got_of(r) for r in results]


def test_a_flagged_job_finishes_on_the_ordinary_path(jobs, golden):
    """RV_MANY_CHAIN_FLAG=5 (test hook): every fifth job of the round counts as flagged by the kernel -- where the reference's trim_overlap would raise -- so its
    anchors are dropped and it runs the ordinary way with the host picker; the results are the same"""
    b = many.Batch()
    b.option("RV_MANY_CHAIN_FLAG", 5)
    kw = dict(cw.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cw.picker_args(kw), chain_wide=True, batch=b)
    flagged = (len(jobs) + 4) // 5
    assert info["shared"] == len(jobs) - flagged and info["ordinary"] == flagged and info["rounds"] == 1
    check_golden(results, golden["default"], "RV_MANY_CHAIN_FLAG=5")
