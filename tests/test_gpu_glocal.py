"""The glocal chain of `reveal transform` on the GPU (rv_glocal.hip): transform.glocalchain_device, glocal_filter and synteny_chain against
tests/golden/glocal.json (the reference's own glocalchain, tools/gen_glocal_golden.py), against the RV_GLOCAL_HOST leg, and as shipped beside the
kernels forced (RV_GLOCAL_HOST_BELOW = 0; the shipped threshold lies above every list, so the default route is the host rule), in both libraries.
Section 3b runs the large cases: lists of 250 .. 2300 blocks, the sizes at which the kernels take their other paths."""
import functools

import pytest

import blocks_cases
import glocal_cases as C
from helpers import feed

pytestmark = pytest.mark.gpu

GOLD = C.golden()
CASES = C.cases()
ADMITTED = [n for n in CASES if n not in C.REFUSED]


def mod(sa64):
    from reveal_amd import reveallib, reveallib64
    return reveallib64 if sa64 else reveallib


def transform():
    from reveal_amd import transform as t
    return t


@functools.lru_cache(maxsize=None)
def lender(sa64, leg):
    """a handle per library and leg whose stream, workspace and switches the calls borrow (never constructed)"""
    idx = mod(sa64).index()
    if leg == "kernels":
        idx.set_option("RV_GLOCAL_HOST_BELOW", 0)
    elif leg == "host":
        idx.set_option("RV_GLOCAL_HOST", 1)
    else:
        assert idx.get_option("RV_GLOCAL_HOST") == 0 and idx.get_option("RV_GLOCAL_HOST_BELOW") > 150
    return idx


def args(c):
    return c["blocks"], c["rlength"], c["qlength"], c["ctg2range"]


# ---- 1. one pass through the kernels against the reference, the host leg and the shipped default
@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("name", ADMITTED)
def test_one_pass(name, axis, sa64):
    t = transform()
    c = CASES[name]
    got, info = t.glocalchain_device(*args(c), axis=axis, sa64=sa64, index=lender(sa64, "kernels"), info=True, **c["kw"])
    assert C.matches(C.indices(c["blocks"], got), GOLD["cases"][name]["axis%d" % axis])
    assert info["route"] == "device"
    host, hinfo = t.glocalchain_device(*args(c), axis=axis, sa64=sa64, index=lender(sa64, "host"), info=True, **c["kw"])
    dflt, dinfo = t.glocalchain_device(*args(c), axis=axis, sa64=sa64, index=lender(sa64, "default"), info=True, **c["kw"])
    assert got == host == dflt and hinfo["route"] == dinfo["route"] == "host"
    if c["blocks"]:
        assert info["passes"] == hinfo["passes"] == ((1, 0) if axis == 0 else (0, 1)) and info["after"] == hinfo["after"] == [len(got)]
        assert info["tiles"] == 1 and info["edges"] >= len(c["blocks"]) and info["chain_blocks"] > len(c["blocks"])
        assert info["sort_keys"] == (2 if name.startswith("wide") else 1)


# ---- 2. the filter: both loops in one call
@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("name", [n for n in C.FILTERED if n not in C.REFUSED])
def test_filter(name, sa64):
    t = transform()
    c = CASES[name]
    want = GOLD["cases"][name]["filter"]
    got, info = t.glocal_filter(*args(c), sa64=sa64, index=lender(sa64, "kernels"), **c["kw"])
    assert C.matches(C.indices(c["blocks"], got), want["chain"])
    host, hinfo = t.glocal_filter(*args(c), sa64=sa64, index=lender(sa64, "host"), **c["kw"])
    dflt, dinfo = t.glocal_filter(*args(c), sa64=sa64, index=lender(sa64, "default"), **c["kw"])
    assert got == host == dflt
    assert info["route"] == "device" and hinfo["route"] == dinfo["route"] == "host"
    if c["blocks"]:
        assert list(info["passes"]) == want["passes"] and info["after"] == want["after"]
        assert info["passes"] == hinfo["passes"] and info["after"] == hinfo["after"]
        assert info["tiles"] == sum(info["passes"]) - info["after"][:-1].count(0)
        assert info["bytes_down"] == 28 * info["tiles"] + 4 * len(got)          # a few counts per pass, the chain once


def test_filter_makes_its_own_handle_and_one_axis():
    t = transform()
    c = CASES["passes_four"]
    want = GOLD["cases"]["passes_four"]["filter"]
    got, info = t.glocal_filter(*args(c), **c["kw"])                              # as shipped: the host rule inside the call
    assert C.matches(C.indices(c["blocks"], got), want["chain"]) and info["route"] == "host"
    first, i0 = t.glocal_filter(*args(c), axes=(0,), index=lender(False, "kernels"), **c["kw"])
    assert i0["route"] == "device" and i0["passes"] == (want["passes"][0], 0)
    second, i1 = t.glocal_filter(first, *args(c)[1:], axes=(1,), index=lender(False, "kernels"), **c["kw"])
    assert second == got and i1["passes"] == (0, want["passes"][1])


# ---- 3. tiles: the same list under a low edge budget
@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("budget", [64, 500, 2048])
def test_tiles(budget, sa64):
    t = transform()
    c = CASES["lastn100_150"]
    idx = mod(sa64).index()
    idx.set_option("RV_GLOCAL_HOST_BELOW", 0)
    idx.set_option("RV_GLOCAL_EDGE_BUDGET", budget)
    for axis in (0, 1):
        one, oinfo = t.glocalchain_device(*args(c), axis=axis, sa64=sa64, index=lender(sa64, "kernels"), info=True, **c["kw"])
        got, info = t.glocalchain_device(*args(c), axis=axis, sa64=sa64, index=idx, info=True, **c["kw"])
        assert got == one and C.matches(C.indices(c["blocks"], got), GOLD["cases"]["lastn100_150"]["axis%d" % axis])
        assert oinfo["tiles"] == 1 and info["edges"] == oinfo["edges"] > 150 * (64 if axis == 0 else 32)      # axis 0: windows of more than 64 edges
        assert info["tiles"] >= 4 and info["tiles"] == info["edges"] // budget + 1          # several tiles, windows crossing their borders
    got, info = t.glocal_filter(*args(c), sa64=sa64, index=idx, **c["kw"])
    assert C.matches(C.indices(c["blocks"], got), GOLD["cases"]["lastn100_150"]["filter"]["chain"]) and info["tiles_max"] >= 4


# ---- 3b. the large cases (glocal_cases.large_cases): more than one workgroup, windows above 192 edges, lists above the 2048 scores of the LDS ring
LARGE = C.large_cases()


@functools.lru_cache(maxsize=None)
def large_lender(sa64, leg, budget=None):
    """a handle per library, leg and edge budget (None: the shipped 2^25)"""
    idx = mod(sa64).index()
    if leg == "kernels":
        idx.set_option("RV_GLOCAL_HOST_BELOW", 0)
    elif leg == "host":
        idx.set_option("RV_GLOCAL_HOST", 1)
    else:
        assert idx.get_option("RV_GLOCAL_HOST") == 0 and idx.get_option("RV_GLOCAL_HOST_BELOW") > 2400
    if budget is None:
        assert idx.get_option("RV_GLOCAL_EDGE_BUDGET") == 1 << 25
    else:
        idx.set_option("RV_GLOCAL_EDGE_BUDGET", budget)
    return idx


@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("name", list(LARGE))
def test_large_one_pass(name, axis, sa64):
    """one pass of the kernels against the reference's record, the host leg and the shipped default; the counts the library reports say that the
    case got where glocal_cases.large_cases sends it (the arithmetic behind them: test_cpu_glocal.py::test_large_reach)"""
    t = transform()
    c = LARGE[name]
    want = GOLD["large"][name]["axis%d" % axis]
    m = C.entries(c, axis)
    got, info = t.glocalchain_device(*args(c), axis=axis, sa64=sa64, index=large_lender(sa64, "kernels"), info=True, **c["kw"])
    assert C.matches(C.indices(c["blocks"], got), want)
    assert info["route"] == "device"
    host, hinfo = t.glocalchain_device(*args(c), axis=axis, sa64=sa64, index=large_lender(sa64, "host"), info=True, **c["kw"])
    dflt, dinfo = t.glocalchain_device(*args(c), axis=axis, sa64=sa64, index=large_lender(sa64, "default"), info=True, **c["kw"])
    assert got == host == dflt and hinfo["route"] == dinfo["route"] == "host"
    assert info["passes"] == hinfo["passes"] == ((1, 0) if axis == 0 else (0, 1)) and info["after"] == hinfo["after"] == [len(got)]
    assert info["tiles"] == 1 and info["chain_blocks"] == m
    assert info["sort_keys"] == (2 if name.startswith("wide") else 1)
    if name in C.WHOLE_PREFIX:
        assert info["edges"] == C.whole_prefix_edges(m)                       # the k-th entry has k edges: every window length 1 .. m is there
    else:
        assert m <= info["edges"] <= C.whole_prefix_edges(m)
    if name.startswith("collinear") and axis == 0:
        assert len(got) == len(c["blocks"])                                   # the longest path a list of this length can have
    for budget in C.LARGE_BUDGETS.get(name, ()):
        low, linfo = t.glocalchain_device(*args(c), axis=axis, sa64=sa64, index=large_lender(sa64, "kernels", budget), info=True, **c["kw"])
        assert low == got and linfo["route"] == "device"
        assert linfo["edges"] == info["edges"] and linfo["tiles"] == linfo["edges"] // budget + 1 > 1
        if name == "ring_2300":
            assert linfo["tiles"] == 6 and C.first_entry_of_tile(5, budget) > C.RING      # the last tile's pre-load starts behind entry 0


@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("name", C.LARGE_FILTERED)
def test_large_filter(name, sa64):
    """both loops: the survivors of a pass compacted into the next pass' list, over more than one workgroup"""
    t = transform()
    c = LARGE[name]
    want = GOLD["large"][name]["filter"]
    got, info = t.glocal_filter(*args(c), sa64=sa64, index=large_lender(sa64, "kernels"), **c["kw"])
    assert C.matches(C.indices(c["blocks"], got), want["chain"])
    host, hinfo = t.glocal_filter(*args(c), sa64=sa64, index=large_lender(sa64, "host"), **c["kw"])
    dflt, dinfo = t.glocal_filter(*args(c), sa64=sa64, index=large_lender(sa64, "default"), **c["kw"])
    assert got == host == dflt
    assert info["route"] == "device" and hinfo["route"] == dinfo["route"] == "host"
    assert list(info["passes"]) == want["passes"] and info["after"] == want["after"]
    assert info["passes"] == hinfo["passes"] and info["after"] == hinfo["after"]
    assert info["tiles"] == sum(info["passes"]) and info["tiles_max"] == 1
    assert info["bytes_down"] == 28 * info["tiles"] + 4 * len(got)
    assert info["sort_keys"] == (2 if name.startswith("wide") else 1)
    if name == "passes_big":
        assert max(info["passes"]) >= 3 and info["after"][0] > C.WG            # a second pass of more than one workgroup


# ---- 4. what the library's arithmetic refuses
def test_refused_takes_python():
    t = transform()
    for name in C.REFUSED:
        c = CASES[name]
        got, info = t.glocal_filter(*args(c), index=lender(False, "kernels"), **c["kw"])
        assert info["route"] == "python" and C.matches(C.indices(c["blocks"], got), GOLD["cases"][name]["filter"]["chain"])
        with pytest.raises(t.error):
            t.glocalchain_device(*args(c), index=lender(False, "kernels"), **c["kw"])
    c = CASES["cross"]
    with pytest.raises(t.error, match="negative weight"):
        t.glocalchain_device(*args(c), index=lender(False, "kernels"), **dict(c["kw"], eps=-1))
    with pytest.raises(t.error, match="ctgid"):
        t.glocalchain_device(c["blocks"] + [(100, 200, 10100, 10200, 0, 50, 0, 1)], *args(c)[1:], index=lender(False, "kernels"), **c["kw"])


# ---- 5. end to end
@pytest.mark.parametrize("sa64", [False, True])
def test_synteny_chain(sa64):
    t = transform()
    ref, ctgs = blocks_cases.multi_case()
    M = blocks_cases.MULTI
    r = t.synteny_chain(ref, ctgs, minctglength=blocks_cases.MULTI_MINCTG, mincluster=M["minclustsize"], minlength=M["minlength"], cluster=M["cluster"],
                        maxdist=M["maxdist"], sa64=sa64)
    blocks, nodes, rlength, qlength = C.multi_blocks()
    want = GOLD["multi"]
    assert r["blocks"] == blocks and r["ctg2range"] == nodes and (r["rlength"], r["qlength"]) == (rlength, qlength)
    assert r["chain"] == [blocks[i] for i in want["chain"]]
    assert list(r["info"]["passes"]) == want["passes"] and r["info"]["after"] == want["after"] and r["info"]["route"] == "host"      # as shipped
    dev, info = t.glocal_filter(r["blocks"], r["rlength"], r["qlength"], r["ctg2range"], sa64=sa64, index=lender(sa64, "kernels"))
    assert dev == r["chain"] and info["route"] == "device" and list(info["passes"]) == want["passes"]


# ---- 6. state: the workspace is shared with getblocks
def test_state():
    t = transform()
    idx = feed(mod(False).index(), blocks_cases.fixture_inputs("1a+1b"))
    idx.set_option("RV_BLOCKS_HOST_BELOW", 0)
    idx.set_option("RV_GLOCAL_HOST_BELOW", 0)
    idx.construct()
    first = idx.getblocks()
    assert len(first) == 73
    ranges = sorted(idx.nodes)
    chain, info = t.glocal_filter(first, idx.nsep[0], idx.n - idx.nsep[0], ranges, index=idx)
    assert info["route"] == "device" and 0 < len(chain) <= 73
    assert chain == t.glocal_filter(first, idx.nsep[0], idx.n - idx.nsep[0], ranges, route="python")[0]
    assert idx.getblocks() == first
    assert t.glocal_filter(first, idx.nsep[0], idx.n - idx.nsep[0], ranges, index=idx)[0] == chain
