"""tests/construct_paths_cases.py is what it claims to be -- shown with the oracle alone, no GPU and no library: the exact n on either side of
the size thresholds, the copy counts as sizes of LCP intervals, the largest common prefixes, the bytes below the separator, the flagged
characters' positions modulo the packed text's block, and (once, from the recorded digests) the two large inputs of D11."""
import importlib.util
import json
import os

import numpy as np
import pytest

import construct_paths_cases as C
from helpers import GOLD, ROOT, oracle


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(cid):
        if cid not in cache:
            c = C.case(cid)
            T, nsep = C.text_of(c)
            cache[cid] = (c, T, nsep, oracle(False).construct(T, nsep, len(c["samples"])))
        return cache[cid]
    return get


def test_every_decision_has_both_sides():
    cs = C.small_cases()
    assert {c["decision"] for c in cs} == {"D1", "D2", "D4", "D5", "D6", "D7", "D8", "D9", "D10", "D12"}
    for c in cs:
        assert set(c["expect"]) <= set(C.FIELDS), c["id"]
    n = {c["id"]: c["claim"]["n"] for c in cs}
    assert sorted(v for k, v in n.items() if k.startswith("D1_") and k.endswith(("1024", "1025"))) == [1024] * 7 + [1025] * 6
    assert n["D1_single_2"] == 2 and n["D1_pair_9"] == 9
    assert (n["D6_indel_4095"], n["D6_indel_4096"]) == (4095, 4096)
    assert sorted(v for k, v in n.items() if k.startswith("D8_")) == [8192] * 3 + [8193] * 3
    assert all(v > C.TINY_MAX for k, v in n.items() if k.startswith(("D7_", "D9_", "D12_", "D4_", "D5_", "D6_")))
    assert all(v < 10 ** 4 for k, v in n.items() if k.startswith("D7_copies")) and all(v < 10 ** 5 for k, v in n.items() if k.startswith("D7_spread"))
    assert all(v < 10 ** 6 for v in n.values())


@pytest.mark.parametrize("cid", C.small_ids())
def test_case_is_what_it_claims(built, cid):
    c, T, nsep, r = built(cid)
    claim = c["claim"]
    assert len(T) == claim["n"] and len(nsep) == len(c["samples"]) - 1
    SA, SAi, LCP = r["SA"], r["SAi"], r["LCP"]
    assert np.array_equal(np.sort(SA), np.arange(len(T)))
    if "copies" in claim:             # the LCP interval of the 120-mer holds exactly c ranks
        kmer, cnt = claim["copies"]
        at = T.find(kmer.encode())
        lo = hi = int(SAi[at])
        while LCP[lo] >= len(kmer):
            lo -= 1
        while hi + 1 < len(T) and LCP[hi + 1] >= len(kmer):
            hi += 1
        assert hi - lo + 1 == cnt and T.count(kmer.encode()) == cnt
        if cid.startswith("D7_spread"):
            assert all(sum(x.count(kmer) for x in s) == 1 for s in c["samples"])
        else:
            assert sum(x.count(kmer) for x in c["samples"][0]) == cnt
    if "maxlcp" in claim:
        assert int(LCP.max()) == claim["maxlcp"]
    if "below_sep" in claim:
        assert len({b for b in T if b < ord("$")}) == claim["below_sep"]
    if claim.get("empty"):
        assert b"$$" in T
    else:
        assert b"$$" not in T
    if "ncount" in claim:             # D10: single N, more than a window of the far round apart, the last one a window in front of the separator
        at = [p for p in range(nsep[0]) if T[p] == ord("N")]
        assert 2 * len(at) == claim["ncount"] == T.count(b"N")
        assert all(b - a > C.TEXT_LIM for a, b in zip(at, at[1:])) and nsep[0] - at[-1] > C.TEXT_LIM and at[0] > C.TEXT_LIM
        assert T[:nsep[0]] == T[nsep[0] + 1:-1]
    if "special" in claim:            # D12
        pos, what = claim["special"]
        ch = T[pos:pos + 1]
        assert (ch == b"N") if what == "N" else (ch == b"$") if what == "border" else (ch.islower() and ch.upper() in b"ACGT")
        if claim["last"]:
            assert pos // C.PK_BLOCK == (len(T) - 1) // C.PK_BLOCK
        else:
            assert pos in (127, 128, 129) and pos % C.PK_BLOCK in (127, 0, 1)
        # the samples agree for more than 200 bases on either side of it (as far as the sample goes), but for the character itself
        starts = [0] + [s + 1 for s in nsep]
        k = max(j for j, s in enumerate(starts) if s <= pos)
        off = pos - starts[k]
        for j, s in enumerate(starts):
            if j != k:
                L = len(T) // len(starts) - 1
                lo, hi = max(0, off - 201), min(L, off + 202)
                assert T[s + lo:s + off].upper() == T[pos - (off - lo):pos].upper() and T[s + off + 1:s + hi].upper() == T[pos + 1:pos + hi - off].upper()
                assert off - lo > 120 and (hi - off > 200 or claim["last"])


def test_derived_layouts_are_the_documented_ones():
    """the restated key layout (construct_paths_cases.key_layout) gives the layouts rv_construct.hip's comments state for plain DNA"""
    # five-letter DNA whose last byte is the separator: radix 5; "seventeen symbols in 5 x 7 + 5 = 40 bits" at 5 x 10^8 (rv_construct.hip:352-353, :2541-2542)
    assert C.key_layout(5, 5, 500_000_002, 1) == (3, 17, 40)
    # without the shorter alphabet a sixth value: three digits need eight bits, "15 instead of 17" in the same 40 bits (:2541-2542)
    assert 5 * 8 == 40 and C._bitlen(6 ** 3 - 1) == 8 and C._bitlen(5 ** 3 - 1) == 7


def test_large_cases_match_their_recorded_digests():
    """D11, once: the inputs have the common prefix they claim, and tests/golden/construct_paths.json is what the oracle gives for them"""
    spec = importlib.util.spec_from_file_location("gen_construct_paths_golden", os.path.join(ROOT, "oracle", "gen_construct_paths_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLD, "construct_paths.json")) as f:
        gold = json.load(f)
    assert sorted(gold) == sorted(C.LARGE_IDS)
    for cid, E in zip(C.LARGE_IDS, (C.LL_LIMIT - 1, C.LL_LIMIT)):
        rec, _ = gen.record(cid)
        assert rec["maxlcp"] == E == C.case(cid)["claim"]["maxlcp"]
        assert rec["n"] == 2 * E + 155 + 1 + 1000 + 1
        for k, v in rec.items():
            assert gold[cid][k] == v, (cid, k)
