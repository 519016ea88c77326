"""Both sides of every decision rv_build_sa takes on the host (tests/construct_paths_cases.py): per case and library
width SA, LCP, the largest LCP (SAi and SO with more than two samples) and the match list equal the oracle's, exactly, and the census of the
build (index.sa_paths()) says that the side the case was built for is the side that ran.  Then the switches that select other kernels in
this build, on the small case of the decision each governs: the same arrays, and a census that differs from the default's in the field the
switch governs and in what follows from it, nowhere else."""
import json
import os

import numpy as np
import pytest

import construct_paths_cases as C
from helpers import GOLD, csr_tuples, oracle

pytestmark = pytest.mark.gpu

CENSUS = {}      # (case id, sa64, switches) -> sa_paths() of every build this module made: the coverage test at the end reads it
_REF = {}


def mod(sa64):
    from reveal_amd import reveallib, reveallib64
    return reveallib64 if sa64 else reveallib


def reference(cid):
    """the oracle's arrays and match list for a case, made once (the 32-bit oracle: both libraries must give these values)"""
    if cid not in _REF:
        c = C.case(cid)
        T, nsep = C.text_of(c)
        k = len(c["samples"])
        O = oracle(False)
        r = O.construct(T, nsep, k)
        ref = dict(T=T, nsep=nsep, SA=r["SA"], LCP=r["LCP"], SAi=r["SAi"], SO=r["SO"], maxlcp=int(r["LCP"].max()), mums=None)
        if k == 2:
            l, a, b = O.getmums(r["tbuf"], r["SA"], r["LCP"], nsep, 20)
            ref["mums"] = [(int(l[i]), (int(a[i]), int(b[i])), 0) for i in range(len(l))]
        elif k > 2:
            ref["mums"] = csr_tuples(*O.getmultimums(r["tbuf"], r["SA"], r["LCP"], r["SO"], nsep, k, 12, 2))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[cid] = ref
    return _REF[cid]


def build(cid, sa64=False, switches=()):
    c = C.case(cid)
    idx = mod(sa64).index()
    for name, value in switches:
        idx.set_option(name, value)
    C.feed_case(idx, c)
    try:
        idx.construct()
    except Exception as e:      # a device error ends the session: nothing more is started on a device that has faulted
        if "hip" in str(e).lower() or "illegal" in str(e).lower():
            pytest.exit("device error in construct() of %s %r: %s" % (cid, switches, e), returncode=3)
        raise
    CENSUS[(cid, sa64, tuple(switches))] = idx.sa_paths()
    return c, idx


def check_arrays(idx, cid, tag=None):
    c, ref = C.case(cid), reference(cid)
    tag = (cid, tag, idx.sa_paths())
    assert idx.n == len(ref["T"]) and idx.nsep == ref["nsep"], tag
    assert idx.T.encode("latin-1") == ref["T"], tag
    assert np.array_equal(idx.array("SA"), ref["SA"]), tag
    assert np.array_equal(idx.array("LCP"), ref["LCP"]), tag
    assert idx.maxlcp == ref["maxlcp"], tag
    k = len(c["samples"])
    if k > 2:
        assert np.array_equal(idx.array("SAi"), ref["SAi"]), tag
        assert np.array_equal(idx.array("SO"), ref["SO"]), tag
        assert idx.getmultimums(12, 2) == ref["mums"], tag
    elif k == 2:
        assert idx.getmums(20) == ref["mums"], tag


def check_census(got, expect, tag):
    assert set(got) == set(C.FIELDS), tag
    assert 0 <= got["defer_max"] <= got["defer_cap"] or got["defer_cap"] == 0 == got["defer_max"], (tag, got)
    for f, want in expect.items():
        if want == ">0":
            assert got[f] > 0, (tag, f, got)
        elif want == "<=cap":
            assert got["defer_max"] <= got["defer_cap"], (tag, f, got)
        else:
            assert got[f] == want, (tag, f, want, got)
    if got["text_round"]:      # rv_construct.hip:2937-2958: the work division follows the hint, the packed text is made whenever the round runs
        assert got["text_mode"] == C.text_mode_of(got) and got["packed_text"] == 1, (tag, got)
    else:
        assert got["text_mode"] == 0 and got["packed_text"] == 0 and got["text_big"] == 0 and got["far_ran"] == 0 and got["defer_cap"] == 0, (tag, got)
    if got["tiny"]:
        assert all(got[f] == 0 for f in C.FIELDS if f not in ("tiny", "fused_asked", "fused_final")), (tag, got)


@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("cid", C.small_ids())
def test_case(cid, sa64):
    c, idx = build(cid, sa64)
    check_arrays(idx, cid)
    check_census(idx.sa_paths(), c["expect"], cid)


@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("cid", C.LARGE_IDS)
def test_large_case(cid, sa64):
    """D11: a common prefix of 2^21 - 1 bases is the longest k_lcp_list finishes; at 2^21 it raises its flag and the whole index goes through
    rv_build_lcp.  4.2 x 10^6 positions: compared with the oracle's recorded digests (tests/golden/construct_paths.json)"""
    with open(os.path.join(GOLD, "construct_paths.json")) as f:
        gold = json.load(f)[cid]
    c, idx = build(cid, sa64)
    got = idx.sa_paths()
    assert idx.n == gold["n"]
    assert C.digest(idx.array("SA")) == gold["sha_SA"], got
    assert C.digest(idx.array("LCP")) == gold["sha_LCP"], got
    assert idx.maxlcp == gold["maxlcp"] == c["claim"]["maxlcp"], got
    m = idx.getmums(20)
    mums = np.array([(l, a, b) for l, (a, b), _ in m], dtype=np.int64).reshape(-1, 3)
    assert len(m) == gold["mums"] and C.digest(mums) == gold["sha_mums"], got
    check_census(got, c["expect"], cid)


# ---- the switches ------------------------------------------------------------------------------------------------------------------------
# what a switch may change in the census besides the field it governs: what the code derives from that field
_HINT_OFF = {"nd_bits", "collapse", "heads_kernel", "text_mode", "far_ran", "nd_table", "diag_table_tried", "diag_table_kept", "defer_max", "defer_cap"}
_NO_TEXT = {"text_round", "text_mode", "packed_text", "text_big", "far_ran", "nd_table", "text_jump", "slow_class", "defer_max", "defer_cap", "doubling_rounds"}
SWITCHES = {
    # name: (switches, cases, fields that must take these values, fields that may differ from the default build's)
    "no_tiny_sa": ((("RV_NO_TINY_SA", 1),), [i for i in C.small_ids() if i.startswith("D1_") and i.endswith("_1024")] + ["D1_pair_9"] +
                   [i for i in C.small_ids() if i.startswith("D2_") and i.endswith("_small")], dict(tiny=0), set(C.FIELDS)),
    "no_short_alphabet": ((("RV_NO_SHORT_ALPHABET", 1),), ["D2_dna_3000", "D2_two_letters_3000", "D2_one_letter_3000"], dict(short_alphabet=0, ends_with_sep=0),
                          {"short_alphabet", "ends_with_sep", "g", "K", "bits", "nd_bits", "defer_max", "defer_cap", "doubling_rounds"}),
    "no_diag": ((("RV_NO_DIAG", 1),), ["D4_family_2", "D4_family_3", "D4_family_16"], dict(nd_bits=0, collapse=0, heads_kernel=0), _HINT_OFF),
    "no_packed_text": ((("RV_NO_PACKED_TEXT", 1),), ["D12_N_128_all_3", "D12_border_127_all_3", "D12_lower_129_one_3", "D12_N_last_all_2", "D4_family_17"],
                       dict(packed_text=0, nd_bits=0, collapse=0), _HINT_OFF | {"packed_text"}),
    "no_heads_fusion": ((("RV_NO_HEADS_FUSION", 1),), ["D4_family_2", "D4_family_3"], dict(heads_kernel=0, collapse=0),
                        {"heads_kernel", "collapse", "diag_table_tried", "diag_table_kept", "defer_max", "defer_cap"}),
    # (the pairs no longer finished by the head kernels lengthen the text round's list; its work list is counted per region of workgroups)
    "no_pub_twins": ((("RV_NO_PUB_TWINS", 1),), ["D4_family_2", "D4_family_3", "D12_N_128_all_2"], dict(), {"defer_max", "defer_cap"}),
    "sa_no_text": ((("RV_SA_NO_TEXT", 1),), ["D7_copies_5", "D7_copies_9", "D7_spread_9", "D4_family_3"], dict(text_round=0, doubling_rounds=">0"), _NO_TEXT),
    "text_mode_0": ((("RV_TEXT_MODE", 0),), [i for i in C.small_ids() if i.startswith("D7_")], dict(text_round=1, text_mode=0), {"text_mode", "defer_max", "defer_cap"}),
    "text_mode_2": ((("RV_TEXT_MODE", 2),), [i for i in C.small_ids() if i.startswith("D7_")], dict(text_round=1, text_mode=2), {"text_mode", "defer_max", "defer_cap"}),
    "no_fused_lcp": ((("RV_NO_FUSED_LCP", 1),), [i for i in C.small_ids() if i.startswith("D7_")], dict(fused_asked=0, fused_final=0, nd_bits=0),
                     _HINT_OFF | {"fused_asked", "fused_final"}),
    # the build leaves LCP to rv_build_lcp only without the fused path (or behind k_lcp_list's overflow, 4 x 10^6 positions: too slow rank by rank)
    "lcp_by_rank": ((("RV_NO_FUSED_LCP", 1), ("RV_LCP_BY_RANK", 1)), ["D7_copies_5", "D12_N_128_all_3", "D12_border_127_all_3"],
                    dict(fused_final=0, lcp_by_rank=1), _HINT_OFF | {"fused_asked", "fused_final", "lcp_by_rank"}),
    "lcp_by_rank_unused": ((("RV_LCP_BY_RANK", 1),), ["D7_copies_5"], dict(fused_final=1, lcp_by_rank=0), set()),
}
_DERIVE_ARG = {"no_tiny_sa": "no_tiny", "no_short_alphabet": "no_short", "no_diag": "no_diag", "no_packed_text": "no_packed", "no_heads_fusion": "no_heads_fusion",
               "no_fused_lcp": "no_fused", "lcp_by_rank": "no_fused"}


@pytest.mark.parametrize("name,cid", [(name, cid) for name, spec in SWITCHES.items() for cid in spec[1]])
def test_switch(name, cid):
    switches, _, must, may = SWITCHES[name]
    if (cid, False, ()) not in CENSUS:
        build(cid)
    base = CENSUS[(cid, False, ())]
    c, idx = build(cid, False, switches)
    check_arrays(idx, cid, name)
    got = idx.sa_paths()
    for f, want in must.items():
        assert (got[f] > 0) if want == ">0" else (got[f] == want), (name, cid, f, got)
    if name in _DERIVE_ARG:      # the fields that follow from the text's statistics, restated with the switch
        T, nsep = C.text_of(c)
        for f, want in C.derive(T, nsep, **{_DERIVE_ARG[name]: True}).items():
            assert got[f] == want or (f == "lcp_by_rank" and name == "lcp_by_rank"), (name, cid, f, want, got)
    changed = {f for f in C.FIELDS if got[f] != base[f]}
    assert changed <= may, (name, cid, sorted(changed - may), base, got)
    governed = [f for f, want in must.items() if want != ">0" and base[f] != want]
    assert governed or name in ("no_pub_twins", "lcp_by_rank_unused") or (name == "no_tiny_sa" and base["tiny"] == 1), (name, cid, base, got)
    assert 0 <= got["defer_max"] <= max(got["defer_cap"], 0)


def test_every_side_of_every_decision_ran():
    """across the module's builds every census field takes each of its values: a decision nobody reached fails here by name"""
    for cid in C.small_ids() + list(C.LARGE_IDS):
        if (cid, False, ()) not in CENSUS:
            build(cid)
    for name, cid in (("text_mode_0", "D7_copies_9"), ("text_mode_2", "D7_copies_9"), ("no_fused_lcp", "D7_copies_9"), ("lcp_by_rank", "D7_copies_5")):
        if (cid, False, SWITCHES[name][0]) not in CENSUS:
            build(cid, False, SWITCHES[name][0])
    if ("D9_partners_4096", False, (("RV_FAR_TABLE", 1),)) not in CENSUS:      # the table of k_far_nd: by itself only from 2^21 tied entries on
        c, idx = build("D9_partners_4096", False, (("RV_FAR_TABLE", 1),))
        check_arrays(idx, "D9_partners_4096", "far_table")
    seen = {f: set() for f in C.FIELDS}
    default = {f: set() for f in C.FIELDS}
    for (cid, sa64, sw), p in CENSUS.items():
        for f in C.FIELDS:
            seen[f].add(p[f])
            if not sw:
                default[f].add(p[f])
    # what the default build decides from its input
    for f in ("tiny", "short_alphabet", "ends_with_sep", "fused_final", "collapse", "diag_table_tried", "diag_table_kept", "text_round", "packed_text",
              "text_big", "far_ran", "slow_class", "text_jump", "lcp_list_overflow"):
        assert default[f] == {0, 1}, (f, default[f])
    assert default["heads_kernel"] == {0, 1, 2} and default["text_mode"] == {0, 1, 3}, default
    assert {0, 2, 3, 8, 9, 16} <= default["hint_ns"] and max(default["hint_ns"]) == 16, default["hint_ns"]
    assert 0 in default["nd_bits"] and max(default["nd_bits"]) > 0
    assert 0 in default["doubling_rounds"] and max(default["doubling_rounds"]) > 1
    assert 0 in default["defer_max"] and max(default["defer_max"]) > 0 and max(default["defer_cap"]) > 0
    assert len(default["g"] - {0}) >= 3 and len(default["K"]) >= 5 and len(default["bits"]) >= 5, default
    # what only a switch (or an input of 2^21 tied suffixes, or a key above 48 bits) reaches
    assert seen["fused_asked"] == {0, 1} and seen["nd_table"] == {0, 1} and seen["lcp_by_rank"] == {0, 1} and seen["text_mode"] == {0, 1, 2, 3}, seen
