"""getblocks' rule on the CPU: the Python restatement (reveal_amd.transform.blocks_python) and the library's host C++ (blocks_native, rv_blocks_host:
no device is asked for) against tests/golden/blocks.json, which tools/gen_blocks_golden.py wrote from the reference's own addctginfo +
clustermumsbydiagonal; and the unique-key claim behind the rule's total order on every oracle list."""
import functools

import pytest

import blocks_cases as C
from reveal_amd import transform

GOLD = C.golden()
ABSTRACT = C.abstract_cases()


@functools.lru_cache(maxsize=None)
def oracle_list(name, minlength, rc):
    inputs = C.multi_inputs() if name == "multi" else C.fixture_inputs(name)
    return C.oracle_mums(inputs, minlength, rc)


def both(mums, ranges, rc, kw, rec):
    for fn, more in ((transform.blocks_python, {}), (transform.blocks_native, dict(sa64=False)), (transform.blocks_native, dict(sa64=True))):
        if rec.get("error"):
            with pytest.raises(transform.error, match="overlapping matches on a diagonal"):
                fn(list(mums), ranges, rcmums=bool(rc), **kw, **more)
            continue
        got = fn(list(mums), ranges, rcmums=bool(rc), **kw, **more)
        assert C.matches_golden(got, rec), (fn.__name__, more, len(got))
        assert all(b[4] == rc for b in got)


@pytest.mark.parametrize("rc", [0, 1])
@pytest.mark.parametrize("name", list(C.FIXTURES))
def test_fixtures_match_the_reference(name, rc):
    for vname, v in C.VARIANTS.items():
        p = C.params(**v)
        mums, ranges = oracle_list(name, p["minlength"], rc)
        rec = GOLD["fixtures"]["%s|rc%d|%s" % (name, rc, vname)]
        assert len(mums) == rec["mums"]
        assert C.keys_unique(mums, rc)
        both(mums, ranges, rc, dict(cluster=p["cluster"], maxdist=p["maxdist"], minclustsize=p["minclustsize"]), rec)


def test_fixture_counts():
    """553 MUMs -> 73 blocks, largest score 13 965, on 1a+1b forward and on its mirror image; two rc MUMs of 1a+1b give no block"""
    for key in ("1a+1b|rc0|defaults", "1a+1brc|rc1|defaults"):
        rec = GOLD["fixtures"][key]
        assert (rec["mums"], rec["count"], rec["largest_score"]) == (553, 73, 13965)
    assert GOLD["fixtures"]["1a+1b|rc1|defaults"] == dict(mums=2, blocks=[])
    assert GOLD["fixtures"]["1a+1b|rc0|minlength_huge"] == dict(mums=0, blocks=[])


@pytest.mark.parametrize("rc", [0, 1])
def test_several_sequences_per_sample(rc):
    mums, ranges = oracle_list("multi", C.MULTI["minlength"], rc)
    rec = GOLD["multi"]["rc%d" % rc]
    assert len(mums) == rec["mums"] > 0 and len(rec["blocks"]) > 0
    assert len(ranges) == 6 and C.keys_unique(mums, rc)
    both(mums, ranges, rc, dict(cluster=True, maxdist=C.MULTI["maxdist"], minclustsize=C.MULTI["minclustsize"]), rec)
    assert len({(b[6], b[7]) for b in rec["blocks"]}) > 1      # more than one pair of sequences


@pytest.mark.parametrize("name", list(ABSTRACT))
def test_abstract_lists_match_the_reference(name):
    c = ABSTRACT[name]
    both(c["mums"], c["ranges"], c["rc"], c["kw"], GOLD["abstract"][name])


def test_abstract_expectations():
    """what the hand-made lists are there for, spelled out"""
    g = GOLD["abstract"]
    assert len(g["dist_eq_maxdist"]["blocks"]) == 2 and len(g["dist_maxdist_minus1"]["blocks"]) == 1
    assert g["dist_maxdist_minus1"]["blocks"][0] == [10, 119, 2010, 2119, 0, 80, 0, 2]
    assert len(g["score_eq_min"]["blocks"]) == 1 and g["score_min_minus1"]["blocks"] == []
    assert [b[6:] for b in g["split_contigs"]["blocks"]] == [[0, 2], [0, 3]]
    assert [b[6:] for b in g["split_refs"]["blocks"]] == [[0, 2], [1, 2]]
    # all five on one diagonal: a position on a '$' belongs to the sequence it ends, the next one to the next sequence; (1000, 3000) and (1011, 3011) merge
    assert [b[:2] + b[6:] for b in g["at_end_plus_1"]["blocks"]] == [[0, 10, 0, 2], [999, 1009, 0, 2], [1000, 1021, 1, 3], [1999, 2009, 1, 3]]
    assert g["rc_pair"]["blocks"] == [[100, 150, 2470, 2520, 1, 40, 0, 2]]
    assert g["overlap"].get("error") and len(g["overlap_other_ids"]["blocks"]) == 2
    assert g["empty"]["blocks"] == []
    assert g["one_diagonal_merged"]["blocks"] == [[0, 15 * 4999 + 10, 100001, 100001 + 15 * 4999 + 10, 0, 50000, 0, 1]]
    assert g["one_diagonal_maxdist0"]["count"] == 5000
