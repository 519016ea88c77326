"""CPU suite: the inputs of the mums_many tests (tests/many_mums_cases.py) can catch what they are meant to catch -- conditions on the CPU
oracle, not measurements --, `many.takes_shared_scan` follows the admission rule of csrc/rv_many.hip, and the argument errors of `mums_many`
come before anything asks for a device."""
import pytest

import many_mums_cases as C
from reveal_amd import many


def test_takes_shared_scan_follows_the_admission_rule():
    """2 .. 64 sequences, at most 2048 ranks, no NUL byte: both sides of every bound"""
    t = many.takes_shared_scan
    assert t([b"A", b"C"])
    assert not t([b"A"])
    assert t([b"A" * 1023, b"C" * 1023]) and not t([b"A" * 1024, b"C" * 1023])           # 2048 | 2049 ranks
    assert t([b"A" * 31] * 64) and not t([b"A" * 30] * 65)                                 # 64 | 65 sequences (2048 | 2015 ranks)
    assert t([b"A" * 20] * 17) and t([b"A" * 20] * 3)
    assert not t([b"AC\0GT", b"ACGT"])
    for name, seqs in C.corner_jobs():
        assert t([s.encode("latin-1") for s in seqs]), name
    for name, seqs in C.ordinary_jobs():
        assert not t([s.encode("latin-1") for s in seqs]), name
    for fam in C.multi_batch() + C.pair_batch() + C.wide_batch():
        assert t([s.encode("latin-1") for s in fam])


def test_mums_many_argument_errors_need_no_device():
    assert hasattr(many, "mums_many") and hasattr(many.Batch, "scan") and hasattr(many.Batch, "matches")
    with pytest.raises(many.error):
        many.mums_many("ACGT")
    with pytest.raises(many.error):
        many.mums_many([["ACGT", "ACGT"]], kind="mems")
    with pytest.raises(many.error):
        many.mums_many([["ACGT", "ACGT"]], minlength=-1)
    with pytest.raises(many.error):
        many.mums_many([["ACGT"]])
    with pytest.raises(many.error):
        many.mums_many([["ACGT", ""]])


def test_matches_gives_the_references_shapes():
    """Matches builds a job's list from the CSR: (l, (a, b), 0) for getmums, (l, n, ((sample, pos), ..)) for getmultimums"""
    import numpy as np
    arrays = (np.array([0, 1, 3]), np.array([20, 7, 5], np.uint32), np.array([2, 3, 2], np.int32), np.array([0, 2, 5, 7]),
              np.array([0, 1, 2, 0, 1, 1, 2], np.uint16), np.array([3, 40, 9, 1, 5, 6, 12]))
    m = many.Matches(arrays, [True, False])
    assert len(m) == 2 and m.arrays is arrays
    assert m[0] == [(20, (3, 40), 0)]
    assert m[1] == [(7, 3, ((2, 9), (0, 1), (1, 5))), (5, 2, ((1, 6), (2, 12)))]
    assert list(m) == [m[0], m[1]] and m[-1] == m[1]
    with pytest.raises(IndexError):
        m[2]


def test_multi_batch_holds_shared_closing_ranks_subsets_and_full_matches():
    """minlength 20, minn 2: at least 50 records that share their closing rank with another record (a rank that emits several intervals), 100 on a
    sample subset and 50 on all samples; families of k = 3, 4, 5, 8 and 16"""
    batch = C.multi_batch()
    assert {len(f) for f in batch} == {3, 4, 5, 8, 16}
    share = sub = full = 0
    for fam in batch:
        recs = C.oracle_matches(fam, "multimums", 20, 2)
        cr = C.closing_ranks(fam, recs)
        share += sum(1 for u in cr if cr.count(u) > 1)
        sub += sum(1 for r in recs if r[1] < len(fam))
        full += sum(1 for r in recs if r[1] == len(fam))
    assert share >= 50 and sub >= 100 and full >= 50, (share, sub, full)


def test_pair_batch_has_matches_in_most_jobs():
    batch = C.pair_batch()
    assert len(batch) == 44
    assert sum(1 for p in batch if C.oracle_matches(p, "mums", 20)) >= 30
    # getmultimums on a pair index gives getmums' records (the members in SA order)
    for minl in (20, 1):
        for p in batch:
            a, b = C.oracle_matches(p, "mums", minl), C.oracle_matches(p, "multimums", minl)
            assert [(l, n, tuple(sorted(mem))) for l, n, mem in b] == list(a)


def test_wide_batch_has_subset_and_full_matches_in_every_job():
    batch = C.wide_batch()
    assert [len(f) for f in batch] == [17, 24, 32, 33, 48, 64]
    sub = full = 0
    for fam in batch:
        recs = C.oracle_matches(fam, "multimums", 20, 2)
        assert len(recs) > 0, len(fam)
        sub += sum(1 for r in recs if r[1] < len(fam))
        full += sum(1 for r in recs if r[1] == len(fam))
    assert sub > 0 and full > 0, (sub, full)


def test_every_job_follows_the_order_rule_under_the_oracle():
    """the oracle's emission order is closing rank ascending, then l descending: what the threads of the scan kernel give, rank by rank"""
    jobs = C.multi_batch() + C.pair_batch() + C.wide_batch() + [s for _, s in C.corner_jobs() + C.ordinary_jobs()]
    for seqs in jobs:
        for minl in (20, 5, 1):
            assert C.follows_order_rule(seqs, C.oracle_matches(seqs, "multimums", minl, 2)), (len(seqs), minl)


def test_corner_jobs_are_what_their_names_say():
    corner = dict(C.corner_jobs())
    # the last rank of the nested job closes three intervals, all of them matches
    recs = C.oracle_matches(C.NESTED_LAST, "multimums", 1, 2)
    cr = C.closing_ranks(C.NESTED_LAST, recs)
    last = C.ranks(C.NESTED_LAST) - 1
    assert [(r[0], r[1]) for r, u in zip(recs, cr) if u == last] == [(3, 2), (2, 3), (1, 4)]
    # one match, at job-local position 0
    for name in ("match_at_position_0", "match_at_position_0_inner"):
        recs = C.oracle_matches(corner[name], "mums", 20)
        assert len(recs) == 1 and recs[0][2][0] == (0, 0), name
    # maximal through N / lower case only; the control extends one base to the left
    assert [r[0] for r in C.oracle_matches(corner["maximal_through_N"], "mums", 20)] == [25]
    assert 25 in [r[0] for r in C.oracle_matches(corner["maximal_through_lower"], "mums", 20)]
    assert [r[0] for r in C.oracle_matches(corner["not_maximal"], "mums", 20)] == [26]
    assert [(r[0], r[1]) for r in C.oracle_matches(corner["maximal_through_sep_three"], "multimums", 20)] == [(25, 2)]
    # a sample twice in an interval: the tandem family loses matches that its unit would give
    assert len(C.oracle_matches(corner["identical_five"], "multimums", 20)) == 1
    assert C.oracle_matches(corner["two_single_bases"], "auto", 0) == ()
    sizes = {name: C.ranks(s) for name, s in C.corner_jobs()}
    for n in (511, 512, 513, 2047, 2048):
        assert sizes["pair_ranks_%d" % n] == n and sizes["three_ranks_%d" % n] == n
    assert sorted(len(s) for name, s in C.corner_jobs() if name.startswith("k")) == [2, 3, 16, 17, 32, 33, 63, 64]
    ordinary = dict(C.ordinary_jobs())
    assert C.ranks(ordinary["pair_ranks_2049"]) == 2049 and C.ranks(ordinary["pair_ranks_3000"]) == 3000 and len(ordinary["k65"]) == 65
    assert any("\0" in s for s in ordinary["nul_byte"]) and [len(s) for s in ordinary["three_by_1000"]] == [1000] * 3
