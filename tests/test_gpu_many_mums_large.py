"""GPU suite: `many.mums_many(.., large=True)` / RV_MANY_SCAN_LARGE -- the MUM and multi-MUM lists of jobs above 2048 ranks through shared launches
(csrc/rv_many.hip many_round_scan with `large`, csrc/rv_many_large.hip rv_many_large_build_c, csrc/rv_many_scan.hip) -- against the CPU oracle on every
job ALONE (tests/many_mums_cases.py oracle_matches / oracle_arrays), record for record and member for member, in the oracle's order.  Never against the
ordinary path alone, never against mums_many itself.  RV_MANY_SCAN_LARGE_MIN is 1 except where the threshold is the subject."""
import random

import numpy as np
import pytest

import many_cases as mc
import many_multi_cases as mm
import many_mums_cases as C
import many_mums_large_cases as L
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

pytestmark = pytest.mark.gpu


def as_bytes(jobs):
    return [[s.encode("latin-1") for s in seqs] for seqs in jobs]


def batch(sa64=False, large_min=1, **options):
    b = many.Batch(sa64)
    b.option("RV_MANY_SCAN_LARGE_MIN", large_min)
    for name, value in options.items():
        b.option(name, value)
    return b


def scan(jobs, minlength=20, minn=2, kind="auto", sa64=False, batch=None, **kw):
    return many.mums_many(jobs, minlength=minlength, minn=minn, kind=kind, sa64=sa64, toupper=False, batch=batch, **kw)


def check(jobs, matches, kind="auto", minl=20, minn=2):
    """every job's list equals the oracle's: the same records in the same order, the same members in the same order"""
    for j, seqs in enumerate(jobs):
        want = C.oracle_matches(seqs, kind, minl, minn)
        got = C.job_records(matches.arrays, j)
        assert got == want, (j, len(seqs), C.ranks(seqs), got[:3], want[:3])


def same_arrays(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def predicted(jobs, **kw):
    return sum(1 for seqs in as_bytes(jobs) if many.takes_shared_scan(seqs, **kw))


def shuffled(jobs, seed=1):
    jobs = list(jobs)
    random.Random(seed).shuffle(jobs)
    return jobs


def few_thousand():
    """every case but the two at the bound RV_MANY_LARGE_MAX"""
    return L.jobs(without=L.BOUNDS)


@pytest.mark.parametrize("sa64", [False, True])
def test_every_job_equals_the_oracle_in_one_mixed_call(sa64):
    jobs = shuffled(L.jobs())
    m, info = scan(jobs, sa64=sa64, batch=batch(sa64), large=True)
    print("info", info)
    check(jobs, m)
    shared = predicted(jobs, large=True)
    assert info["jobs"] == len(jobs) and info["shared"] == shared and info["ordinary"] == len(jobs) - shared == 3
    assert info["rounds"] >= 2      # the small jobs' round and the large jobs'
    for j, seqs in enumerate(jobs):      # the reference's shapes, on demand
        want = C.oracle_matches(seqs)
        if len(seqs) == 2:
            assert m[j] == [(l, (mem[0][1], mem[1][1]), 0) for l, _, mem in want]
        else:
            assert m[j] == [(l, n, mem) for l, n, mem in want]


def test_switch_off_changes_nothing():
    jobs = shuffled(few_thousand(), 2)
    plain, i_plain = many.mums_many(jobs, toupper=False)
    off, i_off = scan(jobs, batch=batch(), large=False)
    assert i_off == i_plain and same_arrays(off.arrays, plain.arrays)
    small = predicted(jobs)
    assert i_off["shared"] == small and i_off["ordinary"] == len(jobs) - small      # the large jobs count as ordinary
    assert i_off["ordinary"] == sum(1 for s in jobs if L.is_large(s)) and i_off["rounds"] == 1
    check(jobs, off)
    on, i_on = scan(jobs, batch=batch(), large=True)
    assert i_on["shared"] == predicted(jobs, large=True) > small and same_arrays(on.arrays, off.arrays)


def test_threshold_both_sides():
    jobs = shuffled(few_thousand(), 3)
    small = predicted(jobs)
    nlarge = predicted(jobs, large=True) - small
    assert nlarge > 10
    at, i_at = scan(jobs, batch=batch(large_min=nlarge), large=True)
    above, i_above = scan(jobs, batch=batch(large_min=nlarge + 1), large=True)
    assert i_at["shared"] == small + nlarge and i_at["ordinary"] == len(jobs) - small - nlarge
    assert i_above["shared"] == small and i_above["ordinary"] == len(jobs) - small
    assert same_arrays(at.arrays, above.arrays)
    check(jobs, at)
    check(jobs, above)


def test_options_and_environment(monkeypatch):
    jobs = [s for s in few_thousand() if L.is_large(s)][:5]
    b = many.Batch()
    with pytest.raises(many.error, match="RV_MANY_SCAN_LARGE_MIN"):
        b.option("RV_MANY_SCAN_LARGE_MIN", -1)
    _, info = scan(jobs, batch=b, large=True)                        # the default threshold (4) admits five
    assert info["shared"] == 5 == predicted(jobs, large=True)
    _, info = scan(jobs[:many.SCAN_LARGE_MIN - 1], batch=b)          # ... and leaves three ordinary; large=None leaves the switch on
    assert info["shared"] == 0 and info["ordinary"] == many.SCAN_LARGE_MIN - 1
    _, info = scan(jobs[:many.SCAN_LARGE_MIN], batch=b)
    assert info["shared"] == many.SCAN_LARGE_MIN
    monkeypatch.setenv("RV_MANY_SCAN_LARGE", "1")                    # a new Batch reads both names from the environment
    monkeypatch.setenv("RV_MANY_SCAN_LARGE_MIN", "2")
    m, info = scan(jobs[:2])
    assert info["shared"] == 2 and info["ordinary"] == 0
    check(jobs[:2], m)
    monkeypatch.setenv("RV_MANY_SCAN_LARGE_MIN", "3")
    m, info = scan(jobs[:2])
    assert info["shared"] == 0 and info["ordinary"] == 2
    check(jobs[:2], m)


def test_kinds_minn_and_minlength():
    jobs = few_thousand()
    b = batch()
    wide = [s for s in jobs if len(s) > 2 and L.is_large(s)]
    m, info = scan(wide, kind="mums", batch=b, large=True)           # a job of k > 2: sample 0 against the rest
    check(wide, m, "mums")
    assert info["shared"] == predicted(wide, large=True) == len(wide) - 1      # (k65)
    pairs = [s for s in jobs if len(s) == 2 and L.is_large(s)]
    m, info = scan(pairs, kind="multimums", batch=b, large=True)     # members in SA order
    check(pairs, m, "multimums")
    assert info["shared"] == len(pairs) - 1                          # (the NUL byte)
    for j, p in enumerate(pairs):                                    # getmultimums on a pair job: getmums' records
        assert tuple((l, n, tuple(sorted(mem))) for l, n, mem in C.job_records(m.arrays, j)) == C.oracle_matches(p, "mums", 20)
    fam = mm.sized_job(random.Random(8), 8, 2600, 0.02)
    nested = dict((n, list(s)) for n, s, _ in L.large_cases())["nested_last_rank"]
    counts = []
    for minn in (2, 3, 8, 9):
        m, info = scan([fam, nested], minlength=5, minn=minn, kind="multimums", batch=b, large=True)
        check([fam, nested], m, "multimums", 5, minn)
        assert info["shared"] == 2
        counts.append(len(m[0]))
    assert counts[0] >= counts[1] >= counts[2] > 0 and counts[3] == 0, counts
    some = shuffled(jobs, 4)[:16] + [nested]
    res = {}
    for minl in (0, 1, 20, 1 << 20):
        res[minl], _ = scan(some, minlength=minl, batch=b, large=True)
        check(some, res[minl], minl=minl)
    assert same_arrays(res[0].arrays, res[1].arrays)                 # a match has l > 0
    assert all(x == [] for x in res[1 << 20])


def test_results_do_not_depend_on_the_path():
    jobs = shuffled(L.jobs(), 5)
    b = batch()
    shared, info = scan(jobs, batch=b, large=True)
    assert info["ordinary"] == 3
    b.option("RV_MANY_SCAN_ORDINARY", 1)
    ordinary, info = scan(jobs, batch=b)
    assert info["shared"] == 0 and info["ordinary"] == len(jobs) and info["rounds"] == 0
    assert same_arrays(shared.arrays, ordinary.arrays)
    check(jobs, shared)


def test_rounds_split_the_large_jobs():
    jobs = shuffled(few_thousand(), 6)
    rng = random.Random(10)
    a = mc.rnd(rng, 12500)
    jobs.append([a, mc.mutate(rng, a, 0.01)])                        # 25 002 ranks: larger than a round below
    whole, i_whole = scan(jobs, batch=batch(), large=True)
    nsmall = predicted(jobs)
    nlarge = predicted(jobs, large=True) - nsmall
    assert i_whole["rounds"] == 2 and i_whole["shared"] == nsmall + nlarge
    total = sum(C.ranks(s) for s in jobs[:-1] if L.is_large(s) and many.takes_shared_scan(as_bytes([s])[0], large=True))
    lim = total // 3
    assert C.ranks(jobs[-1]) > lim > max(C.ranks(s) for s in jobs[:-1])
    cut, i_cut = scan(jobs, batch=batch(RV_MANY_ROUND=lim), large=True)
    print("info", i_whole, i_cut)
    small_rounds = -(-sum(C.ranks(s) for s in jobs if not L.is_large(s)) // lim)
    assert i_cut["rounds"] >= small_rounds + 3
    assert i_cut["shared"] == nsmall + nlarge - 1 and i_cut["ordinary"] == i_whole["ordinary"] + 1      # the job larger than a round: the ordinary way
    assert same_arrays(whole.arrays, cut.arrays)
    check(jobs, cut)


def test_launches_do_not_grow_with_the_jobs():
    """four large jobs and the same four ten times over, each call one round: the same launches.  Both rounds hold more than 2^15 ranks -- from there on
    (up to 2^26) the sums over the radix sort's histograms take one number of launches, as the sums over the ranks do between 2^11 and 2^22 --, and
    the doubling rounds are the same: they follow the longest repeat, which repeating the jobs does not change"""
    rng = random.Random(4)
    once = [mm.sized_job(rng, k, 9000 + k, 0.01) for k in (2, 3, 8, 17)]
    tenfold = once * 10
    assert 1 << 15 < sum(C.ranks(s) for s in once) and sum(C.ranks(s) for s in tenfold) < 1 << 22
    b = batch()
    m1, i1 = scan(once, batch=b, large=True)
    m10, i10 = scan(tenfold, batch=b, large=True)
    print("info", i1, i10)
    assert i1["shared"] == 4 and i10["shared"] == 40 and i1["ordinary"] == i10["ordinary"] == 0
    assert i1["rounds"] == i10["rounds"] == 1
    assert i1["launches"] == i10["launches"] > 0
    check(once, m1)
    check(tenfold, m10)


@pytest.mark.parametrize("sa64", [False, True])
def test_kept_arrays_of_the_large_jobs(sa64):
    jobs = [list(s) for _, s, shared in L.large_cases() if shared and L.is_large(s)]
    b = batch(sa64, RV_MANY_KEEP=1)
    m, info = scan(jobs, sa64=sa64, batch=b, large=True)
    assert info["shared"] == len(jobs)
    check(jobs, m)
    for j, seqs in enumerate(jobs):
        sa, lcp = b.arrays(j)
        osa, olcp = C.oracle_arrays(seqs)
        assert np.array_equal(sa.astype(np.int64), osa.astype(np.int64)) and np.array_equal(lcp.astype(np.int64), olcp.astype(np.int64)), j


def test_a_reused_batch():
    jobs = shuffled([list(s) for n, s, shared in L.large_cases() if shared and n not in L.BOUNDS], 7)[:12] + C.pair_batch()[:4]
    b = batch()
    first, i1 = scan(jobs, batch=b, large=True)
    check(jobs, first)
    b.run(20, 2)                                            # the same jobs: a scan leaves text and jobs untouched
    head, l, off, pos = b.anchors()
    ref, _ = many.align_many(as_bytes(jobs), toupper=False)
    for j in range(len(jobs)):      # (the order of a job's anchors is launch by launch: the lists are compared sorted, as everywhere)
        assert sorted((int(l[k]), tuple(int(x) for x in pos[off[k]:off[k + 1]])) for k in range(head[j], head[j + 1])) == sorted(ref[j]["anchors"])
        assert b.text(j).decode("latin-1") == ref[j]["T"]
    b.scan(20, 2, "auto")                                   # (the switch stays as the batch has it)
    assert same_arrays(first.arrays, b.matches())
    again, i2 = scan(jobs, batch=b)
    assert same_arrays(first.arrays, again.arrays) and i1 == i2
    assert i1["shared"] == predicted(jobs, large=True)
