"""The five device pickers of align_many at the bounds they admit a job up to (reveal_amd/many.py `chain=`, `chain_multi=`, `chain_wide=`, `chain_large=`,
`chain_large_multi=`; csrc/rv_leaf_chain.hip, rv_leaf_multi_chain.hip, rv_pick_chain.hip, rv_pick_multi_chain.hip and the admission rules of
csrc/rv_many.hip): the jobs of tests/many_chain_limits_cases.py under weights at each class' bound W -- chain scores of up to 2^26 .. 2^29.7 where no other
test goes beyond 2^17 -- and at sizes of exactly 2048, 2^17 and 2^17 + 1 ranks, with relative positions that set bit 16 on either path and in the first
and the last sample.  Every result is compared with tests/golden/many_chain_limits.json (`rem.align` of the job ALONE on the reference's own index),
never with another align_many run."""
import pytest

import many_chain_limits_cases as lm
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

pytestmark = pytest.mark.gpu

ALL_ON = dict(chain=True, chain_multi=True, chain_wide=True, chain_large=True, chain_large_multi=True)
# the built-in picker's switches: on in the ordinary-path runs, where they must mean nothing under a picker
BUILT_IN = dict(multi=True, large=True, large_multi=True, wide=True)


@pytest.fixture(scope="module")
def golden():
    return lm.load_golden()[0]


def as_bytes(job):
    return [s.upper().encode() for s in job]


def got_of(r):
    return sorted((int(l), tuple(int(p) for p in pos)) for l, pos in r["anchors"]), lm.sha(r["T"])


def check_golden(results, want, what):
    bad = [(j, got_of(r)[0][:3], want[j][0][:3]) for j, r in enumerate(results) if got_of(r) != want[j]]
    assert not bad, "%s: %d jobs differ from rem.align on the reference's index, first: %r" % (what, len(bad), bad[:3])


def calls_of(cls):
    """the calls of a class -> [(job indices, fillers in front, big)]: every job below 2^17 ranks in one call; for a large class a second one with its
    jobs of 2^17, 2^17 and 2^17 + 1 ranks behind two small fillers (four admitted jobs: the class' threshold)"""
    n = len(lm.jobs(cls))
    small = [j for j in range(n) if not lm.is_big(cls, j)]
    big = [j for j in range(n) if lm.is_big(cls, j)]
    return [(small, [], False)] + ([(big, lm.fillers(cls), True)] if big else [])


def run(cls, name, golden, sa64=False, want=None, **switches):
    """the class' calls under a set -> [info]; every job is compared with the golden result of set `want` (the set's own unless given); the fillers of
    the second call of a large class are the class' first two jobs, compared under the set's weights as well"""
    jobs = [f for _, f in lm.jobs(cls)]
    infos = []
    for which, fill, big in calls_of(cls):
        kw = dict(lm.sets(cls, big=big))[name]
        results, info = many.align_many(fill + [jobs[j] for j in which], sa64=sa64, picker=lm.picker_args(kw), **switches, **lm.run_kw(kw))
        print("info", cls, name, info)
        res = golden[cls][want or name]
        check_golden(results, [res[j] for j in range(len(fill))] + [res[j] for j in which], "%s %s" % (cls, name))
        infos.append(info)
    return infos


ON_SETS = lm.SET_NAMES[:-1]
CASES = [(cls, n, False) for cls in lm.CLASSES for n in ON_SETS] + [(cls, n, True) for cls in lm.CLASSES for n in ("wmax", "pen-max")]


@pytest.mark.parametrize("cls,name,sa64", CASES)
def test_every_job_equals_the_reference_through_the_shared_launches(golden, cls, name, sa64):
    """every admitted job shares its launches and none is flagged -- a kernel that bails out instead of computing fails here --, the job of 2^17 + 1
    ranks alone comes back from the ordinary path, inside the call whose other jobs share launches"""
    infos = run(cls, name, golden, sa64=sa64, **lm.switch(cls))
    for (which, fill, big), info in zip(calls_of(cls), infos):
        over = 1 if big else 0
        assert info["jobs"] == len(which) + len(fill) and info["ordinary"] == over and info["shared"] == len(which) + len(fill) - over, (big, info)


@pytest.mark.parametrize("cls,name", [(cls, n) for cls in lm.CLASSES for n in ON_SETS])
def test_every_job_equals_the_reference_on_the_ordinary_path(golden, cls, name):
    """the class' switch off, every other one on: the host's 64-bit path -- where the shared launches disagree with the file, this says which is right"""
    infos = run(cls, name, golden, **dict(ALL_ON, **{cls: False}), **BUILT_IN)
    for (which, fill, big), info in zip(calls_of(cls), infos):
        assert info["shared"] == 0 and info["ordinary"] == len(which) + len(fill), (big, info)


@pytest.mark.parametrize("cls", lm.CLASSES)
def test_weights_one_above_the_bound_are_not_admitted(golden, cls):
    """the `over` set, (W + 1, W + 1), with every chain switch on: the admission rules of csrc/rv_many.hip at their bound -- nothing shares a launch, and
    the results are `default`'s (a common factor of both weights changes no decision)"""
    kw = dict(lm.sets(cls))["over"]
    assert (kw["wscore"], kw["wpen"]) == (lm.wmax(cls) + 1,) * 2
    for info in run(cls, "over", golden, want="default", **ALL_ON):
        assert info["shared"] == 0 and info["ordinary"] == info["jobs"], info


@pytest.mark.parametrize("cls", lm.LARGE_CLASSES)
def test_the_jobs_of_2_17_ranks(golden, cls):
    """one call with the two jobs of exactly 2^17 ranks, the job of 2^17 + 1 and two fillers: the anchors that come back through the shared launches lie
    at positions, relative to their sequence's begin, of 2^16 and beyond -- on path 0 / in sample 0 in the job whose long sequence is the first, on path
    1 / in the last sample in the one whose long sequence is the last -- and the job of 2^17 + 1 ranks is the only one that runs the ordinary way"""
    which, fill, big = calls_of(cls)[1]
    jobs = [f for _, f in lm.jobs(cls)]
    batch = fill + [jobs[j] for j in which]
    kw = dict(lm.sets(cls, big=True))["default"]
    args = lm.picker_args(kw)
    takes = [many.takes_shared_launch(as_bytes(f), picker=args, minlength=kw["minlength"], **lm.switch(cls)) for f in batch]
    assert takes == [True] * 4 + [False] and [sum(map(len, f)) + len(f) for f in batch[2:]] == [1 << 17, 1 << 17, (1 << 17) + 1]
    results, info = many.align_many(batch, picker=args, **lm.switch(cls), **lm.run_kw(kw))
    print("info", info)
    assert info["shared"] == 4 and info["ordinary"] == 1
    check_golden(results, [golden[cls]["default"][j] for j in (0, 1)] + [golden[cls]["default"][j] for j in which], cls)
    first, last = (lm.relative_positions(batch[x], got_of(results[x])[0]) for x in (2, 3))
    assert first[0] >= 1 << 16 and max(first[1:]) < 1 << 16, first
    assert last[-1] >= 1 << 16 and max(last[:-1]) < 1 << 16, last
    assert len(last) == (2 if cls == "chain_large" else 16)
