"""index.getblocks / reveal_amd.transform on the GPU: the diagonal clusters of `reveal transform` (transform.py:252-293) with the MUMs kept in device
memory, against the Python restatement over index.getmums, tests/golden/blocks.json (the reference's own functions, tools/gen_blocks_golden.py), the CPU
oracle and the RV_BLOCKS_HOST leg.  A list of fewer than RV_BLOCKS_HOST_BELOW records takes the host rule by default: the tests force the kernels
(RV_BLOCKS_HOST_BELOW = 0), force the host leg (RV_BLOCKS_HOST = 1) and run the shipped default beside them."""
import functools

import numpy as np
import pytest

import blocks_cases as C
import dense_cases as dc
from helpers import assemble, feed, oracle

pytestmark = pytest.mark.gpu

GOLD = C.golden()
ABSTRACT = C.abstract_cases()


def mod(sa64):
    from reveal_amd import reveallib, reveallib64
    return reveallib64 if sa64 else reveallib


def transform():
    from reveal_amd import transform as t
    return t


@functools.lru_cache(maxsize=None)
def lender(sa64):
    """one handle per library whose stream and workspace the abstract lists borrow (never constructed)"""
    return mod(sa64).index()


# ---- 1. fixtures against the oracle + golden
@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("rc", [0, 1])
@pytest.mark.parametrize("name", list(C.FIXTURES))
def test_fixtures(name, rc, sa64):
    t = transform()
    idx = feed(mod(sa64).index(), C.fixture_inputs(name))
    ranges = sorted(idx.nodes)
    idx.set_option("RV_BLOCKS_HOST_BELOW", 0)                            # the kernels whatever the record count
    idx.construct(rc=rc)
    host = feed(mod(sa64).index(), C.fixture_inputs(name))
    host.set_option("RV_BLOCKS_HOST", 1)
    host.construct(rc=rc)
    dflt = feed(mod(sa64).index(), C.fixture_inputs(name))               # as shipped: these lists lie below the threshold
    assert dflt.get_option("RV_BLOCKS_HOST_BELOW") > 553 and dflt.get_option("RV_BLOCKS_HOST") == 0
    dflt.construct(rc=rc)
    lists = {}
    for vname, v in C.VARIANTS.items():
        p = C.params(**v)
        if p["minlength"] not in lists:
            lists[p["minlength"]] = idx.getmums(p["minlength"])
        mums = lists[p["minlength"]]
        rec = GOLD["fixtures"]["%s|rc%d|%s" % (name, rc, vname)]
        args = (p["minlength"], p["cluster"], p["maxdist"], p["minclustsize"])
        got = idx.getblocks(*args)
        assert got == t.blocks_python(mums, ranges, p["cluster"], p["maxdist"], p["minclustsize"], rcmums=bool(rc)), vname
        assert C.matches_golden(got, rec), vname
        assert got == host.getblocks(*args), vname
        assert got == dflt.getblocks(*args), vname
        arr = idx.getblocks_arrays(*args)
        assert arr["o"] == rc and arr["info"]["mums"] == rec["mums"] == len(mums)
        assert arr["info"]["clusters"] >= len(got) and (p["cluster"] or arr["info"]["clusters"] == len(mums))
        assert arr["info"] == host.getblocks_arrays(*args)["info"] == dflt.getblocks_arrays(*args)["info"]
    if (name, rc) in (("1a+1b", 0), ("1a+1brc", 1)):
        d = idx.getblocks_arrays()
        assert (d["info"]["mums"], d["info"]["clusters"], len(d["s1"]), int(d["score"].max())) == (553, 100, 73, 13965)


# ---- 2. several sequences per sample, through synteny_blocks
@pytest.mark.parametrize("sa64", [False, True])
def test_synteny_blocks_several_sequences(sa64):
    t = transform()
    ref, ctgs = C.multi_case()
    r = t.synteny_blocks(ref, ctgs, minctglength=C.MULTI_MINCTG, mincluster=C.MULTI["minclustsize"], sa64=sa64,
                         **{k: C.MULTI[k] for k in ("minlength", "cluster", "maxdist")})
    T, nsep, nodes = assemble(C.multi_inputs())
    assert r["ctg2range"] == nodes and len(nodes) == 6                     # the contig below minctglength is not in it
    assert r["sep"] == nsep[0] == r["rlength"] and r["qlength"] == len(T) - nsep[0]
    assert r["mums"] == (GOLD["multi"]["rc0"]["mums"], GOLD["multi"]["rc1"]["mums"]) and min(r["mums"]) > 0
    want = GOLD["multi"]["rc0"]["blocks"] + GOLD["multi"]["rc1"]["blocks"]
    assert [list(b) for b in r["blocks"]] == want
    assert {b[4] for b in r["blocks"]} == {0, 1}
    # the oracle alone
    both = []
    for rc in (0, 1):
        mums, ranges = C.oracle_mums(C.multi_inputs(), C.MULTI["minlength"], rc, sa64)
        both += t.blocks_python(mums, ranges, True, C.MULTI["maxdist"], C.MULTI["minclustsize"], rcmums=bool(rc))
    assert r["blocks"] == both
    # synteny_blocks ran as shipped (lists this short take the host rule); the same index through the kernels
    idx = feed(mod(sa64).index(), C.multi_inputs())
    idx.set_option("RV_BLOCKS_HOST_BELOW", 0)
    dev = []
    for rc in (0, 1):
        idx.construct(rc=rc)
        dev += idx.getblocks(C.MULTI["minlength"], True, C.MULTI["maxdist"], C.MULTI["minclustsize"])
    assert dev == both


# ---- 3. abstract lists through the kernels
@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("name", list(ABSTRACT))
def test_abstract_lists(name, sa64):
    t = transform()
    c = ABSTRACT[name]
    rec = GOLD["abstract"][name]
    if rec.get("error"):
        with pytest.raises(t.error, match="overlapping matches on a diagonal"):
            t.blocks_device(c["mums"], c["ranges"], rcmums=bool(c["rc"]), sa64=sa64, index=lender(sa64), **c["kw"])
        return
    got = t.blocks_device(c["mums"], c["ranges"], rcmums=bool(c["rc"]), sa64=sa64, index=lender(sa64), **c["kw"])
    assert got == t.blocks_python(c["mums"], c["ranges"], rcmums=bool(c["rc"]), **c["kw"])
    assert C.matches_golden(got, rec)
    if name == "one_diagonal_merged":
        assert len(got) == 1 and got[0][5] == 50000
    if name == "one_diagonal_maxdist0":
        assert len(got) == 5000
    if name == "empty":
        assert got == []


def test_blocks_device_makes_its_own_handle():
    t = transform()
    c = ABSTRACT["rc_three"]
    assert t.blocks_device(c["mums"], c["ranges"], rcmums=True, **c["kw"]) == t.blocks_python(c["mums"], c["ranges"], rcmums=True, **c["kw"])


# ---- 4. the capacity retry under getblocks
def test_capacity_retry():
    t = transform()
    inputs = dc.unrelated_pair()
    T, nsep, nodes = assemble(inputs)
    O = oracle(False)
    c = O.construct(T, nsep, 2)
    l, a, b = O.getmums(c["tbuf"], c["SA"], c["LCP"], nsep, dc.MINL)
    assert len(l) == 6050 > dc.pair_out_cap(len(T)) == 4623
    want = sorted(((int(a[k]), int(a[k] + l[k]), int(b[k]), int(b[k] + l[k]), 0, int(l[k]), 0, 1) for k in range(len(l))), key=lambda x: x[2])
    idx = feed(mod(False).index(), inputs)
    assert 0 < idx.get_option("RV_BLOCKS_HOST_BELOW") < 6050                 # as shipped this list stays on the device
    idx.construct()
    assert idx.getblocks(dc.MINL, cluster=False) == want
    ev = idx.capacity_events()
    assert ev["pair_out"] >= 1
    assert idx.getblocks(dc.MINL, cluster=False) == want
    assert idx.capacity_events() == ev                                   # the second turn finds the list large enough
    mums = [(int(l[k]), (int(a[k]), int(b[k])), 0) for k in range(len(l))]
    assert idx.getblocks(dc.MINL, True, 30, 20) == t.blocks_python(mums, nodes, True, 30, 20)
    # a threshold above the count: the retry runs all the same, then the whole list has arrived with the header and takes the host rule
    low = feed(mod(False).index(), inputs)
    low.set_option("RV_BLOCKS_HOST_BELOW", 10000)
    low.construct()
    assert low.getblocks(dc.MINL, cluster=False) == want
    assert low.capacity_events()["pair_out"] >= 1
    assert low.getblocks(dc.MINL, True, 30, 20) == t.blocks_python(mums, nodes, True, 30, 20)


# ---- 5. state
@pytest.mark.parametrize("below", [0, None])
def test_state(below):
    m = mod(False)
    idx = feed(m.index(), C.fixture_inputs("1a+1b"))
    if below is not None:
        idx.set_option("RV_BLOCKS_HOST_BELOW", below)
    with pytest.raises(TypeError, match="Index not yet constructed."):
        idx.getblocks()
    idx.construct()
    mums = idx.getmums(20)
    first = idx.getblocks()
    assert len(first) == 73 and idx.getmums(20) == mums
    assert idx.getblocks() == first
    arr = idx.getblocks_arrays()
    assert arr["s1"].dtype == np.int64 and arr["refid"].dtype == np.int32 and len(arr["ctgid"]) == 73
    idx.align_builtin(20, 2)
    with pytest.raises(TypeError):
        idx.getblocks()


def test_needs_two_samples():
    m = mod(False)
    idx = m.index()
    idx.addsample("one")
    idx.addsequence("ACGTACGTTGCA")
    idx.construct()
    with pytest.raises(m.error, match="two samples"):
        idx.getblocks()
