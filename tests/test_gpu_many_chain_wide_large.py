"""align_many with the reference's default picker on the device for jobs of 17 .. 64 sequences above 2048 ranks (reveal_amd/many.py `chain_wide_large=`,
csrc/rv_many.hip, the 64-sample form of k_pick_multi_chain in csrc/rv_pick_multi_chain.hip): every job's anchors -- length and members in the order they
are emitted -- and final text against `rem.align` of that job ALONE -- on the reference's own index through tests/golden/many_chain_wide_large.json, or
the product's callback path run here -- the built-in picker against the CPU oracle; never against align_many itself."""
import random

import pytest

import many_chain_cases as cc
import many_chain_large_cases as cp
import many_chain_large_multi_cases as cl
import many_chain_multi_cases as cm
import many_chain_wide_cases as cx
import many_chain_wide_large_cases as cw
import many_multi_cases as mm
import many_wide_cases as mw
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

pytestmark = pytest.mark.gpu

ON = dict(chain_wide_large=True)
# every other switch: none of them takes a job of this class
OTHERS = dict(chain=True, chain_multi=True, chain_wide=True, chain_large=True, chain_large_multi=True, multi=True, large=True, large_multi=True, wide=True)


@pytest.fixture(scope="module")
def jobs():
    return [list(fam) for _, fam in cw.jobs()]


@pytest.fixture(scope="module")
def golden():
    return cw.load_golden()


def as_bytes(job):
    return [s.upper().encode() for s in job]


def got_of(r):
    return sorted((int(l), tuple(int(p) for p in pos)) for l, pos in r["anchors"]), cw.sha(r["T"])


def check_golden(results, want, what):
    bad = [(j, got_of(r)[0][:3], want[j][0][:3]) for j, r in enumerate(results) if got_of(r) != want[j]]
    assert not bad, "%s: %d jobs differ from rem.align on the reference's index, first: %r" % (what, len(bad), bad[:3])


def check_rem_align(jobs, results, kw, which):
    """against the product's own rem.align (Python callbacks on a stand-alone index of the job)"""
    bad = []
    for j in which:
        an, T = cw.rem_align_job(jobs[j], **kw)
        got, sha = got_of(results[j])
        if got != an or sha != cw.sha(T):
            bad.append((j, [len(s) for s in jobs[j]], got[:3], an[:3]))
    assert not bad, "%d jobs differ from rem.align, first: %r" % (len(bad), bad[:3])


CASES = [(n, False) for n, _ in cw.SETS] + [("default", True)]


@pytest.mark.parametrize("name,sa64", CASES)
def test_every_job_equals_the_reference_through_the_shared_launches(jobs, golden, name, sa64):
    kw = dict(cw.SETS)[name]
    results, info = many.align_many(jobs, sa64=sa64, picker=cw.picker_args(kw), **ON, **cw.run_kw(kw))
    print("info", info)
    check_golden(results, golden[name], name)
    assert info["jobs"] == len(jobs) and info["shared"] == len(jobs) and info["ordinary"] == 0 and info["rounds"] == 1


@pytest.mark.parametrize("name,sa64", CASES)
def test_every_job_equals_the_reference_on_the_ordinary_path(jobs, golden, name, sa64):
    kw = dict(cw.SETS)[name]
    # (every other switch on: without the new one none takes a job of 17 .. 64 sequences above 2048 ranks under a picker)
    results, info = many.align_many(jobs, sa64=sa64, picker=cw.picker_args(kw), chain_wide_large=False, **OTHERS, **cw.run_kw(kw))
    print("info", info)
    check_golden(results, golden[name], name)
    assert info["shared"] == 0 and info["ordinary"] == len(jobs)


@pytest.mark.parametrize("sa64", [False, True])
def test_positions_of_17_bits(golden, sa64):
    """the job of 118 517 ranks under its own set (a seedsize and a maxmums that admit it), with small fillers so that the call reaches
    RV_MANY_CHAIN_WIDE_LARGE_MIN: its chain works at positions of the first sequence from 66 000 on"""
    name, kw = cw.BIG_SET
    n = max(many.CHAIN_WIDE_LARGE_MIN - 1, 1)
    batch = [cw.big_job()] + cw.fillers(n)
    args = cw.picker_args(kw)
    assert all(many.takes_shared_launch(as_bytes(j), picker=args, **ON) for j in batch)
    results, info = many.align_many(batch, minlength=kw["minlength"], sa64=sa64, picker=args, **ON)
    print("info", info)
    assert info["shared"] == n + 1 and info["ordinary"] == 0
    assert got_of(results[0]) == golden["big"][0]
    assert any(1 << 16 <= p < 70000 for _, pos in got_of(results[0])[0] for p in pos)
    check_rem_align(batch, results, kw, list(range(1, n + 1)))


def test_more_candidates_than_the_cap_flag_the_job(jobs, golden):
    """RV_PICK_MCHAIN_CAP=8 (test hook; it lowers the cap of either form of the kernel): a sub-index with more than eight candidates flags its job, and
    exactly the jobs the fixture's `roots` and `below` name are flagged -- the most candidates the reference's picker saw at the root and in any
    sub-index below it; the flagged jobs finish on the ordinary path"""
    b = many.Batch()
    b.option("RV_PICK_MCHAIN_CAP", 8)
    kw = dict(cw.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cw.picker_args(kw), batch=b, **ON)
    print("info", info)
    over = [max(r[0], c) > 8 for r, c in zip(golden["roots"], golden["below"])]
    assert 0 < sum(over) < len(jobs)
    assert info["ordinary"] == sum(over) and info["shared"] == len(jobs) - sum(over)
    assert b.flagged() == {32: sum(over)}      # (rv_many_flagged: every one of them by the cap's bit, none by another)
    check_golden(results, golden["default"], "RV_PICK_MCHAIN_CAP=8")
    # ... and which: the jobs the fixture says stay inside the cap, alone, are all shared
    inside = [j for j, o in enumerate(over) if not o]
    results, info = many.align_many([jobs[j] for j in inside], minlength=20, picker=cw.picker_args(kw), batch=b, **ON)
    assert info["shared"] == len(inside) and info["ordinary"] == 0 and b.flagged() == {}
    check_golden(results, [golden["default"][j] for j in inside], "RV_PICK_MCHAIN_CAP=8, the jobs inside the cap")


def test_a_level_without_device_tables_is_picked_by_the_host(jobs, golden):
    """RV_DECIDE_MAX_SUBS=0 (test hook): no level ships the tables of the device-side decisions, so every level's whole match list comes to the host and
    rv_pick_chain decides every sub-index there -- never the longest match, which the fixture's shuffled, tied and subset jobs would show"""
    b = many.Batch()
    b.option("RV_DECIDE_MAX_SUBS", 0)
    kw = dict(cw.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cw.picker_args(kw), batch=b, **ON)
    print("info", info)
    assert info["shared"] == len(jobs) and info["ordinary"] == 0
    check_golden(results, golden["default"], "RV_DECIDE_MAX_SUBS=0")


def test_a_flagged_job_finishes_on_the_ordinary_path(jobs, golden):
    """RV_MANY_CHAIN_FLAG=5 (test hook): every fifth job of the round counts as flagged; the results are the same"""
    b = many.Batch()
    b.option("RV_MANY_CHAIN_FLAG", 5)
    kw = dict(cw.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cw.picker_args(kw), batch=b, **ON)
    flagged = (len(jobs) + 4) // 5
    assert info["shared"] == len(jobs) - flagged and info["ordinary"] == flagged and info["rounds"] == 1
    assert b.flagged() == {16: flagged}
    check_golden(results, golden["default"], "RV_MANY_CHAIN_FLAG=5")


def test_fewer_jobs_than_the_threshold_stay_ordinary(jobs, golden):
    kw = dict(cw.SETS)["default"]
    n = many.CHAIN_WIDE_LARGE_MIN - 1
    assert n >= 1
    sub = jobs[10:10 + n]
    results, info = many.align_many(sub, minlength=20, picker=cw.picker_args(kw), **ON)
    assert info["shared"] == 0 and info["ordinary"] == n
    check_golden(results, golden["default"][10:10 + n], "below RV_MANY_CHAIN_WIDE_LARGE_MIN")
    results, info = many.align_many(sub + [jobs[24]], minlength=20, picker=cw.picker_args(kw), **ON)
    assert info["shared"] == n + 1 and info["ordinary"] == 0
    check_golden(results, golden["default"][10:10 + n] + [golden["default"][24]], "at RV_MANY_CHAIN_WIDE_LARGE_MIN")


def test_launches_do_not_depend_on_the_number_of_jobs(jobs, golden):
    sub = list(range(5, 25))
    b = many.Batch()
    kw = dict(cw.SETS)["default"]
    r1, i1 = many.align_many([jobs[j] for j in sub], minlength=20, picker=cw.picker_args(kw), batch=b, **ON)
    r6, i6 = many.align_many([jobs[j] for j in sub] * 6, minlength=20, picker=cw.picker_args(kw), batch=b, **ON)
    print("info", i1, i6)
    assert i1["shared"] == len(sub) and i6["shared"] == 6 * len(sub) and i1["rounds"] == i6["rounds"] == 1
    assert i1["launches"] == i6["launches"]
    check_golden(r1, [golden["default"][j] for j in sub], "once")
    check_golden(r6, [golden["default"][j] for j in sub] * 6, "six times")


def test_several_rounds(jobs, golden):
    b = many.Batch()
    total = sum(mm.ranks(j) for j in jobs)
    b.option("RV_MANY_ROUND", total // 3)
    kw = dict(cw.SETS)["default"]
    results, info = many.align_many(jobs, minlength=20, picker=cw.picker_args(kw), batch=b, **ON)
    print("info", info)
    assert info["shared"] == len(jobs) and info["ordinary"] == 0 and info["rounds"] >= 3
    check_golden(results, golden["default"], "three rounds")


PICKER_SWITCHES = dict(chain=True, chain_multi=True, chain_wide=True, chain_large=True, chain_large_multi=True, chain_wide_large=True)
EVERY_SWITCH = dict(PICKER_SWITCHES, multi=True, large=True, large_multi=True, wide=True)


def mixed_batch(jobs, golden):
    """small pairs, large pairs, small and large jobs of 3 .. 16 sequences, small jobs of 17 .. 64, this class and a job of 65 sequences, shuffled
    -> (batch, want, position of the job of 65 sequences): want[k] = the golden result of batch[k], None for the job of 65 sequences"""
    small = list(range(0, len(cc.jobs()), 20))
    large = list(range(20, len(cp.jobs()), 10))
    multi = list(range(0, len(cm.jobs()), 16))
    lmulti = list(range(0, len(cl.jobs()), 4))
    wide = list(range(0, len(cx.jobs()), 12))
    mine = list(range(0, len(jobs), 2))
    assert len(large) >= many.CHAIN_LARGE_MIN and len(lmulti) >= many.CHAIN_LARGE_MULTI_MIN and len(mine) >= many.CHAIN_WIDE_LARGE_MIN
    k65 = dict((n, f) for n, f, _ in mw.corner_jobs())["k65"]
    gx = cx.load_golden()["default"]
    batch = ([list(cc.jobs()[j][1]) for j in small] + [list(cp.jobs()[j][1]) for j in large] + [list(cm.jobs()[j][1]) for j in multi] +
             [list(cl.jobs()[j][1]) for j in lmulti] + [list(cx.jobs()[j][1]) for j in wide] + [jobs[j] for j in mine] + [list(k65)])
    want = ([cc.load_golden()["default"][j] for j in small] + [cp.load_golden()["default"][j] for j in large] + [cm.load_golden()["default"][j] for j in multi] +
            [cl.load_golden()["default"][j] for j in lmulti] + [gx[j] for j in wide] + [golden["default"][j] for j in mine] + [None])
    order = list(range(len(batch)))
    random.Random(22).shuffle(order)
    return [batch[k] for k in order], [want[k] for k in order], order.index(len(batch) - 1)


def test_mixed_batch_with_every_switch_on(jobs, golden):
    """the jobs of mixed_batch with every picker switch on: only the job of 65 sequences stays ordinary, info["shared"] is what takes_shared_launch
    says, every class runs one round; a sample against the product's rem.align per job, the rest against the golden files"""
    kw = dict(minlength=20)
    args = cw.picker_args(kw)
    batch, want, at65 = mixed_batch(jobs, golden)
    results, info = many.align_many(batch, minlength=20, picker=args, **EVERY_SWITCH)
    print("info", info)
    takes = [many.takes_shared_launch(as_bytes(j), picker=args, minlength=20, **PICKER_SWITCHES) for j in batch]
    assert sum(takes) == len(batch) - 1 and not takes[at65]
    assert info["shared"] == sum(takes) and info["ordinary"] == 1
    assert info["rounds"] == 6 and info["launches"] == 1108      # a round per class that has jobs; the launches of this batch, as recorded before the class table
    sample = set(random.Random(23).sample(range(len(batch)), 4)) | {k for k, w in enumerate(want) if w is None}
    check_rem_align(batch, results, kw, sorted(sample))
    for k, w in enumerate(want):
        if w is None or k in sample:
            continue
        if isinstance(w, dict):      # (many_chain_wide_cases keeps its results as records)
            assert cx.same(w, *got_of(results[k])), k
        else:
            assert got_of(results[k]) == w, k


def test_the_built_in_picker_is_back_after_a_picker_run(jobs, golden):
    """one Batch: a run with the picker and chain_wide_large, then one without a picker and wide=True -- the second equals the CPU oracle's built-in
    picker and differs from the first on the shuffled, tied and subset jobs"""
    b = many.Batch()
    sub = list(range(0, 25))
    batch = [jobs[j] for j in sub]
    r1, i1 = many.align_many(batch, picker=cw.picker_args(dict(minlength=20)), batch=b, **ON)
    r2, i2 = many.align_many(batch, wide=True, batch=b)
    assert i1["shared"] == len(sub) and i2["shared"] == len(sub) and i1["ordinary"] == i2["ordinary"] == 0
    check_golden(r1, [golden["default"][j] for j in sub], "the picker's run")
    differ = 0
    for k, job in enumerate(batch):
        anchors, T = mm.oracle_job(as_bytes(job), 20)
        got = sorted((int(l), tuple(int(p) for p in pos)) for l, pos in r2[k]["anchors"])
        assert got == sorted((int(l), tuple(int(p) for p in pos)) for l, pos in anchors) and r2[k]["T"].encode("latin-1") == T, k
        differ += sorted((l, tuple(sorted(p))) for l, p in got_of(r1[k])[0]) != got
    assert differ >= 5          # (and the first run did use the other picker)
