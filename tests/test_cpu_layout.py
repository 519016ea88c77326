"""merge_consecutive and the chain's tail of `reveal transform` without a GPU: the Python restatements and the library's host C++ (rv_merge_host,
rv_chainscore_host, rv_optimise_host) against tests/golden/layout.json -- the reference's own functions run by tools/gen_layout_golden.py --, stage
by stage and through transform.chain_tail; what the validation refuses; the route taken for weights the library's integers do not hold."""
import numpy as np
import pytest

import layout_cases as C

GOLD = C.golden()
MERGE = C.merge_cases()
TAIL = C.tail_cases()


def transform():
    from reveal_amd import transform as t
    return t


def tup(rec):
    return [tuple(b) for b in rec]


def columns(t, rows):
    return {k: np.array([r[c] for r in rows], dtype=dt) for c, (k, dt) in enumerate(t._COLS)}


# ---- 1. the merge rule
@pytest.mark.parametrize("name", list(MERGE))
def test_merge_python(name):
    t = transform()
    blocks = C.merge_list(MERGE[name])
    before = list(blocks)
    got = t.merge_consecutive_python(blocks)
    assert blocks == before and got is not blocks
    assert GOLD["merge"][name]["n"] == len(blocks) and C.matches(got, GOLD["merge"][name]["merged"])


@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("name", list(MERGE))
def test_merge_host(name, sa64):
    t = transform()
    c = MERGE[name]
    want = GOLD["merge"][name]["merged"]
    assert C.matches(t.merge_consecutive_native(C.merge_list(c), sa64=sa64), want)
    rows, sel = (c["rows"], np.array(c["sel"], dtype=np.int32)) if "rows" in c else (c["blocks"], None)
    cols, info = t.merge_arrays(columns(t, rows), sel, sa64=sa64, host=True)
    assert C.matches(t._rows(cols), want)
    assert info["route"] == "host" and info["rows_in"] == GOLD["merge"][name]["n"] and info["rows_out"] == len(cols["s1"])
    assert [cols[k].dtype for k, _ in t._COLS] == [np.dtype(dt) for _, dt in t._COLS]


def test_merge_what_the_cases_are_for():
    """each of these lists would merge differently under one wrong reading of the rule"""
    t = transform()
    m = lambda name: t.merge_consecutive_python(C.merge_list(MERGE[name]))
    assert len(m("other_refid_joins")) == 1                                   # refid compared in the join test: 2
    assert len(m("join_o1")) == 1 and len(m("o1_ranks_ascending")) == 2       # the rank step not negated for o = 1: the other way round
    assert m("join_o1")[0][2:4] == (10100, 10360)                             # e2 taken from the tail for o = 1: 10180
    assert len(m("equal_s1_first")) == 3 and len(m("equal_s1_second")) == 1   # an unstable tie
    assert m("scores_2p31")[0][5] == 5 << 31 > 1 << 32                        # a 32-bit score sum
    wide = C.merge_list(MERGE["wide_coordinates"])
    assert max(b[0] for b in wide) >= 1 << 40 and max(b[2] for b in wide) >= 1 << 40 and min(b[0] for b in wide) < 1 << 32


def test_merge_validation():
    t = transform()
    ok = C.merge_list(MERGE["join_o0"])
    bad = lambda k, v: [tuple(v if c == k else x for c, x in enumerate(ok[0])), ok[1]]
    for blocks, what in ((bad(0, -1), "coordinates"), (bad(3, 1 << 61), "coordinates"), (bad(4, 2), "o is 0 or 1"), (bad(5, -1), "negative score"),
                         ([ok[0][:5] + (1 << 61,) + ok[0][6:]] * 2, "total")):
        with pytest.raises(t.error, match=what):
            t.merge_consecutive_native(blocks)
    with pytest.raises(t.error, match="library's integers"):
        t.merge_consecutive_native(bad(1, 1 << 64))
    cols = columns(t, ok)
    with pytest.raises(t.error, match="different lengths"):
        t.merge_arrays(dict(cols, e2=cols["e2"][:1]), host=True)
    for sel in ([0, 2], [-1], [[0, 1]], [0.5]):
        with pytest.raises(t.error, match="sel"):
            t.merge_arrays(cols, np.array(sel), host=True)
    got, info = t.merge_arrays(cols, np.zeros(0, dtype=np.int32), host=True)       # an empty sel is an empty list
    assert len(got["s1"]) == 0 and info["rows_in"] == 0
    got, info = t.merge_arrays(cols, [1, 1, 0], host=True)                          # duplicates are entries of their own
    assert info["rows_in"] == 3 and t._rows(got) == t.merge_consecutive_python([ok[1], ok[1], ok[0]])


# ---- 2. the tail, stage by stage on the reference's own intermediate lists
def args(c):
    return c["rlength"], c["qlength"], c["ctg2range"]


@pytest.mark.parametrize("name", list(TAIL))
def test_tail_stages(name):
    t = transform()
    c, g = TAIL[name], GOLD["tail"][name]
    assert t.merge_consecutive_python(c["chain"]) == tup(g["merged"]) == t.merge_consecutive_native(c["chain"])
    if isinstance(g["overlap"], dict):
        assert g["overlap"]["raises"] in ("IndexError", "AssertionError")
        with pytest.raises(t.error, match="remove_overlap"):
            t.remove_overlap_python(tup(g["merged"]), c["greedy"])
        with pytest.raises(t.error, match="remove_overlap"):
            t.chain_tail(c["chain"], *args(c), greedy=c["greedy"], minchainsum=c["minchainsum"], **c["kw"])
        return
    merged = tup(g["merged"])
    assert t.remove_overlap_python(merged, c["greedy"]) == tup(g["overlap"]) and merged == tup(g["merged"])
    assert [b for b in tup(g["overlap"]) if b[5] >= c["minchainsum"]] == tup(g["filtered"])
    m2 = tup(g["merged2"])
    assert t.merge_consecutive_python(tup(g["filtered"])) == m2 == t.merge_consecutive_native(tup(g["filtered"]))
    for fn in (t.chainscore_python, t.chainscore_native):
        assert list(fn(list(m2), *args(c), **c["kw"])) == g["chainscore"] and len(g["chainscore"][2]) == len(m2) + 1
    if len(m2) > 1:
        for fn in (t.optimise_python, t.optimise_native):
            best, w, cost, edges = fn(sorted(m2, key=lambda s: s[0]), *args(c), **c["kw"])
            assert dict(blocks=[list(b) for b in best], weight=w, cost=cost, edgecosts=edges) == g["sweep"], fn.__name__
        for route in ("python", "host"):
            blocks, w, cost, edges, sweeps = t.optimise_loop(m2, *args(c), route=route, **c["kw"])
            assert dict(blocks=[list(b) for b in blocks], weight=w, cost=cost, edgecosts=edges, sweeps=sweeps) == g["loop"], route
    else:
        assert "sweep" not in g and "loop" not in g
    final = tup(g["final"]["blocks"])
    if isinstance(g["extended"], dict):
        with pytest.raises(t.error, match="extendblocks"):
            t.extendblocks_python(final, c["ctg2range"])
    else:
        assert t.extendblocks_python(final, c["ctg2range"]) == tup(g["extended"]) and final == tup(g["final"]["blocks"])


@pytest.mark.parametrize("route", [None, "python", "host"])
@pytest.mark.parametrize("name", list(TAIL))
def test_chain_tail(name, route):
    t = transform()
    c, g = TAIL[name], GOLD["tail"][name]
    if isinstance(g["overlap"], dict) or isinstance(g.get("extended"), dict):
        with pytest.raises(t.error):
            t.chain_tail(c["chain"], *args(c), greedy=c["greedy"], minchainsum=c["minchainsum"], route=route, **c["kw"])
        return
    before = list(c["chain"])
    r = t.chain_tail(c["chain"], *args(c), greedy=c["greedy"], minchainsum=c["minchainsum"], route=route, **c["kw"])
    assert c["chain"] == before
    assert dict(blocks=[list(b) for b in r["blocks"]], weight=r["weight"], cost=r["cost"], edgecosts=r["edgecosts"]) == g["final"]
    assert r["extended"] == tup(g["extended"])
    st = r["info"]["stages"]
    assert [st[k] for k in ("merged", "overlap", "filtered", "merged2")] == [tup(g[k]) for k in ("merged", "overlap", "filtered", "merged2")]
    assert r["info"]["route"] == ("python" if route == "python" else "host")
    if "loop" in g:
        assert st["optimised"] == tup(g["loop"]["blocks"]) and r["info"]["sweeps"] == g["loop"]["sweeps"]
    else:
        assert "optimised" not in st and r["info"]["sweeps"] == 0
    no = t.chain_tail(c["chain"], *args(c), greedy=c["greedy"], minchainsum=c["minchainsum"], route=route, optimise=False, **c["kw"])
    assert no["info"]["sweeps"] == 0 and [list(b) for b in no["blocks"]] == g["merged2"] and [no["weight"], no["cost"], no["edgecosts"]] == g["chainscore"]


def test_tail_what_the_cases_are_for():
    g = GOLD["tail"]
    raising = [n for n in g if isinstance(g[n]["overlap"], dict) or isinstance(g[n].get("extended"), dict)]
    assert 1 <= len(raising) and 5 * len(raising) <= len(g)
    d = g[C.TAIL_DROPS]
    assert d["loop"]["sweeps"] >= 1 and len(d["loop"]["blocks"]) < len(d["merged2"]) and len(d["sweep"]["blocks"]) < len(d["merged2"])
    assert g[C.TAIL_TWO_SWEEPS]["loop"]["sweeps"] >= 2
    assert any(len(g[n]["overlap"]) < len(g[n]["merged"]) for n in g if not isinstance(g[n]["overlap"], dict))          # a contained block left
    assert any(g[n]["overlap"] != g[n]["merged"] and len(g[n]["overlap"]) == len(g[n]["merged"]) for n in g if not isinstance(g[n]["overlap"], dict))
    assert g["tail_s0_n0_conservative_command"]["final"] == dict(blocks=[], weight=0, cost=g["tail_s0_n0_conservative_command"]["final"]["cost"],
                                                               edgecosts=[g["tail_s0_n0_conservative_command"]["final"]["cost"]])


def test_extendblocks_floor_and_empty_block():
    t = transform()
    ranges = [(0, 4999), (5000, 9999)]
    # half of a negative distance is rounded down, as Python 2 divides: 900 + (300 - 900) // 2 = 600 and 5900 + (5301 - 5900) // 2 = 5600
    a, b = (100, 900, 5100, 5900, 0, 10, 0, 1), (300, 950, 5301, 5950, 0, 10, 0, 1)
    assert t.extendblocks_python([b, a], ranges) == [(0, 600, 5000, 5600, 0, 10, 0, 1), (600, 4999, 5600, 9999, 0, 10, 0, 1)]
    # the block in the middle begins where its extended neighbour ends (600) and ends at 400 + (410 - 400) // 2: the reference's assert
    with pytest.raises(t.error, match="extendblocks: an empty block on the reference axis"):
        t.extendblocks_python([a, (300, 400, 6000, 6100, 0, 10, 0, 1), (410, 500, 6200, 6300, 0, 10, 0, 1)], ranges)
    assert t.extendblocks_python([], ranges) == []


# ---- 3. weights the library's integers do not hold
def test_refused_weights_take_python():
    t = transform()
    c = TAIL[C.TAIL_DROPS]
    for kw in (dict(c["kw"], eps=1.5), dict(c["kw"], rearrangecost=1 << 61)):
        r = t.chain_tail(c["chain"], *args(c), **kw)
        assert r["info"]["route"] == "python"
        assert r["blocks"] == t.chain_tail(c["chain"], *args(c), route="python", **kw)["blocks"]
        with pytest.raises(t.error, match="integer arithmetic"):
            t.chain_tail(c["chain"], *args(c), route="host", **kw)
        with pytest.raises(t.error, match="integer arithmetic"):
            t.chainscore_native(c["chain"], *args(c), **kw)
        with pytest.raises(t.error, match="integer arithmetic"):
            t.optimise_native(c["chain"], *args(c), **kw)
    half = t.chain_tail(c["chain"], *args(c), **dict(c["kw"], eps=2.0))            # 2.0 counts as 2
    assert half["info"]["route"] == "host" and half["blocks"] == t.chain_tail(c["chain"], *args(c), **dict(c["kw"], eps=2))["blocks"]
    with pytest.raises(t.error, match="negative weight"):
        t.chain_tail(c["chain"], *args(c), **dict(c["kw"], gapopen=-1))
    with pytest.raises(t.error, match="unknown route"):
        t.chain_tail(c["chain"], *args(c), route="device")


def test_optimise_host_on_a_long_list():
    """a fragmented draft: the host sweep, which makes its two orders once, against the reference's quadratic one on a list of 400"""
    t = transform()
    blocks = C.runs_of(__import__("random").Random(11), 400, maxrun=3)
    ranges = [(0, 99999), (100000, 199999), (200000, 1199999), (1200000, 2199999), (2200000, 3199999)]
    blocks = [(a, e1, b, e2, o, s, 0, ctg) for a, e1, b, e2, o, s, _, ctg in blocks]
    want = t.optimise_python(blocks, 199999, 3000001, ranges, **C.SMALL)
    assert t.optimise_native(blocks, 199999, 3000001, ranges, **C.SMALL) == want and len(want[0]) < 400
