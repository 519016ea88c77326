"""CPU suite: the inputs of the mums_many tests for jobs above 2048 ranks (tests/many_mums_large_cases.py) are what they claim to be -- conditions
on the CPU oracle, not measurements --, and `many.takes_shared_scan(.., large=True)` follows the admission rule of csrc/rv_many.hip
(many_scan_large_admits)."""
import many_mums_cases as C
import many_mums_large_cases as L
from reveal_amd import many


def as_bytes(seqs):
    return [s.encode("latin-1") for s in seqs]


def test_the_generator_is_deterministic():
    a = L.large_cases()
    L.large_cases.cache_clear()
    b = L.large_cases()
    assert a == b and len({n for n, _, _ in a}) == len(a)


def test_every_case_has_the_size_it_claims():
    cases = {n: s for n, s, _ in L.large_cases()}
    for n in (2049, 2050, 3000):
        assert C.ranks(cases["pair_ranks_%d" % n]) == n and len(cases["pair_ranks_%d" % n]) == 2
        assert C.ranks(cases["three_ranks_%d" % n]) == n and len(cases["three_ranks_%d" % n]) == 3
    for k, n in ((16, 2049), (17, 2500), (33, 3333), (64, 4000)):
        s = cases["k%d_ranks_%d" % (k, n)]
        assert len(s) == k and C.ranks(s) == n
    assert [len(s) for s in cases["identical_pair_1100"]] == [1100, 1100] and cases["identical_pair_1100"][0] == cases["identical_pair_1100"][1]
    assert 2400 <= C.ranks(cases["tandem_family"]) <= 2600 and len(cases["tandem_family"]) == 4
    assert len(set(cases["identical_five"])) == 1 and len(cases["identical_five"]) == 5
    assert [len(s) for s in cases["first_of_one_base"]] == [1, 2100] and [len(s) for s in cases["second_of_one_base"]] == [2100, 1]
    assert sorted(len(s) for s in cases["k64_one_long"]) == [1] * 63 + [2000] and len(cases["k64_one_long"][0]) == 1 and len(cases["k64_one_long"][-1]) == 1
    assert "N" * 12 in cases["long_N_run"][0] and "N" * 12 in cases["long_N_run"][1]
    assert all(s == s.lower() for s in cases["lower_case"])
    assert C.ranks(cases["pair_ranks_large_max"]) == L.LARGE_MAX == many.LARGE_MAX and C.ranks(cases["pair_ranks_large_max_plus_1"]) == L.LARGE_MAX + 1
    assert len(cases["k65"]) == 65 and any("\0" in s for s in cases["nul_byte"])
    # every case but the small controls is above the small rounds' 2048 ranks
    for name, seqs, _ in L.large_cases():
        assert L.is_large(seqs) != name.startswith("small_"), name
    # the job whose match ends at its last '$' is the largest of the shared cases below the bound: last in a round sorted by size
    assert C.ranks(cases["match_at_the_end"]) == max(C.ranks(s) for n, s, sh in L.large_cases() if sh and n not in L.BOUNDS)
    assert C.ranks(cases["small_pair_ranks_2048"]) == 2048 == L.LEAF_RANKS == many.LEAF_RANKS


def test_takes_shared_scan_follows_the_table():
    """with the switch: what the table says; without: as ever -- at most 2048 ranks, 2 .. 64 sequences, no NUL byte"""
    t = many.takes_shared_scan
    for name, seqs, shared in L.large_cases():
        b = as_bytes(seqs)
        assert t(b, large=True) == shared, name
        assert t(b, large=False) == t(b) == (shared and not L.is_large(seqs)), name
    # both sides of every bound of the rule
    assert t([b"A" * 1024, b"C" * 1023], large=True) and not t([b"A" * 1024, b"C" * 1023])                     # 2049 ranks
    assert t([b"A" * 40] * 64, large=True) and not t([b"A" * 40] * 65, large=True)                             # 64 | 65 sequences
    assert not t([b"A" * 1100, b"C" * 500 + b"\0" + b"C" * 500], large=True)
    assert t([b"A" * 2000, b"C" * 1998], large=True, large_max=4000) and not t([b"A" * 2000, b"C" * 1999], large=True, large_max=4000)
    assert t([b"A" * 100, b"C" * 100], large=True, large_max=0)                                                # (the small rounds have no such bound)
    assert many.SCAN_LARGE_MIN == 4


def test_nested_last_rank_job_emits_what_its_comment_says():
    seqs = dict((n, s) for n, s, _ in L.large_cases())["nested_last_rank"]
    assert C.ranks(seqs) > L.LEAF_RANKS and all("T" not in s[:L.NESTED_PAD] for s in seqs)
    recs = C.oracle_matches(seqs, "multimums", 1, 2)
    cr = C.closing_ranks(seqs, recs)
    last = C.ranks(seqs) - 1
    assert [(r[0], r[1]) for r, u in zip(recs, cr) if u == last] == [(3, 2), (2, 3), (1, 4)]


def test_corner_cases_are_what_their_names_say():
    cases = {n: s for n, s, _ in L.large_cases()}
    recs = C.oracle_matches(cases["match_at_position_0"], "mums", 20)
    assert len(recs) == 1 and recs[0][0] == 25 and recs[0][2][0] == (0, 0)
    recs = C.oracle_matches(cases["match_at_the_end"], "mums", 20)      # ... and one that ends at the job's last '$'
    a, b = cases["match_at_the_end"]
    assert [(r[0], r[2][0][1] + r[0], r[2][1][1] + r[0]) for r in recs] == [(30, len(a), len(a) + 1 + len(b))]
    assert [r[0] for r in C.oracle_matches(cases["maximal_through_N"], "mums", 20)] == [25]
    assert 25 in [r[0] for r in C.oracle_matches(cases["maximal_through_lower"], "mums", 20)]
    # the LCP stops at N: no match crosses the run, and none lies inside it
    a = cases["long_N_run"][0]
    n0 = a.index("N" * 12)
    recs = C.oracle_matches(cases["long_N_run"], "mums", 5)
    assert recs and all(r[2][0][1] + r[0] <= n0 or r[2][0][1] >= n0 + 12 for r in recs)
    # the identical pair: one match of the whole sequence -- the deepest doubling the class meets here
    assert [r[0] for r in C.oracle_matches(cases["identical_pair_1100"], "mums", 20)] == [1100]
    assert len(C.oracle_matches(cases["identical_five"], "multimums", 20)) == 1
    # a single base against 2100, either way round: matches of one base at most
    for name in ("first_of_one_base", "second_of_one_base"):
        assert C.oracle_matches(cases[name], "mums", 2) == ()


def test_every_case_follows_the_order_rule_under_the_oracle():
    for name, seqs, _ in L.large_cases():
        for minl in (20, 5):
            assert C.follows_order_rule(seqs, C.oracle_matches(seqs, "multimums", minl, 2)), (name, minl)
