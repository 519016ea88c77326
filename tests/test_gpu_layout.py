"""merge_consecutive of `reveal transform` on the GPU (rv_merge.hip) and the layout pipeline on columns: transform.merge_consecutive_device and
merge_arrays against tests/golden/layout.json (the reference's own merge_consecutive, tools/gen_layout_golden.py), with the kernels forced
(RV_MERGE_HOST_BELOW = 0), on the RV_MERGE_HOST leg and as shipped, in both libraries; transform.synteny_layout against synteny_chain + chain_tail
on tuples."""
import functools

import numpy as np
import pytest

import blocks_cases
import layout_cases as C

pytestmark = pytest.mark.gpu

GOLD = C.golden()
MERGE = C.merge_cases()
ROW = 5 * 8 + 3 * 4          # bytes of a row over the eight columns


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
        idx.set_option("RV_MERGE_HOST_BELOW", 0)
    elif leg == "host":
        idx.set_option("RV_MERGE_HOST", 1)
    else:
        assert idx.get_option("RV_MERGE_HOST") == 0
    return idx


def bits(v):
    return max(int(v).bit_length(), 1)


def columns(t, rows):
    return {k: np.array([r[c] for r in rows], dtype=dt) for c, (k, dt) in enumerate(t._COLS)}


# ---- 1. every merge case through the kernels, the host leg and the shipped default
@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("name", list(MERGE))
def test_merge(name, sa64):
    t = transform()
    blocks = C.merge_list(MERGE[name])
    want = GOLD["merge"][name]
    got, info = t.merge_consecutive_device(blocks, sa64=sa64, index=lender(sa64, "kernels"), info=True)
    assert C.matches(got, want["merged"])
    host, hinfo = t.merge_consecutive_device(blocks, sa64=sa64, index=lender(sa64, "host"), info=True)
    dflt, dinfo = t.merge_consecutive_device(blocks, sa64=sa64, index=lender(sa64, "default"), info=True)
    assert got == host == dflt and hinfo["route"] == "host"
    assert lender(sa64, "default").get_option("RV_MERGE_HOST_BELOW") == C.HOST_BELOW
    assert dinfo["route"] == ("host" if len(blocks) < C.HOST_BELOW else "device")
    for i in (info, hinfo, dinfo):
        assert i["rows_in"] == want["n"] == len(blocks) and i["rows_out"] == len(got)
    if len(blocks) < 2:
        assert info["route"] == "host"                                          # nothing to merge: no kernel runs
        return
    assert info["route"] == "device"
    assert info["key_bits"] == (bits(max(b[0] for b in blocks)), bits(max(b[2] for b in blocks)))
    assert info["bytes_up"] == ROW * len(blocks) and info["bytes_down"] == 4 + ROW * len(got)
    assert info["launches"] == 6 and info["kernel_ms"] > 0
    assert hinfo["bytes_up"] == hinfo["bytes_down"] == hinfo["launches"] == 0
    if name == "wide_coordinates":
        assert info["key_bits"][0] > 40 and info["key_bits"][1] > 41


# ---- 2. columns with sel
@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("name", [n for n in MERGE if "rows" in MERGE[n]])
def test_merge_arrays_sel(name, sa64):
    t = transform()
    c = MERGE[name]
    cols, sel = columns(t, c["rows"]), np.array(c["sel"], dtype=np.int32)
    got, info = t.merge_arrays(cols, sel, sa64=sa64, index=lender(sa64, "kernels"))
    assert C.matches(t._rows(got), GOLD["merge"][name]["merged"])
    assert [got[k].dtype for k, _ in t._COLS] == [np.dtype(dt) for _, dt in t._COLS]
    assert info["route"] == "device" and info["rows_in"] == len(sel) and info["rows_out"] == len(got["s1"])
    assert info["bytes_up"] == ROW * len(c["rows"]) + 4 * len(sel) and info["launches"] == 7            # the gather in front
    host, hinfo = t.merge_arrays(cols, sel, sa64=sa64, index=lender(sa64, "host"))
    cpu, cinfo = t.merge_arrays(cols, sel, sa64=sa64, host=True)
    for k, _ in t._COLS:
        assert np.array_equal(got[k], host[k]) and np.array_equal(got[k], cpu[k])
    assert hinfo["route"] == cinfo["route"] == "host" and hinfo["rows_in"] == cinfo["rows_in"] == len(sel)
    # every row, in the order of the rows: sel = None and sel = 0 .. n - 1 are the same list
    every, einfo = t.merge_arrays(cols, None, sa64=sa64, index=lender(sa64, "kernels"))
    ident, iinfo = t.merge_arrays(cols, np.arange(len(c["rows"]), dtype=np.int32), sa64=sa64, index=lender(sa64, "kernels"))
    assert t._rows(every) == t._rows(ident) == t.merge_consecutive_python(c["rows"]) and (einfo["launches"], iinfo["launches"]) == (6, 7)


def test_merge_refuses_on_the_device_leg_too():
    t = transform()
    ok = C.merge_list(MERGE["join_o0"])
    with pytest.raises(t.error, match="o is 0 or 1"):
        t.merge_consecutive_device([ok[0][:4] + (2,) + ok[0][5:], ok[1]], index=lender(False, "kernels"))
    with pytest.raises(t.error, match="sel"):
        t.merge_arrays(columns(t, ok), np.array([0, 2]), index=lender(False, "kernels"))
    assert t.merge_consecutive_device(ok) == t.merge_consecutive_python(ok)          # its own handle, as shipped


# ---- 3. the pipeline on columns against the one on tuples
def pairs():
    ref, ctgs = blocks_cases.multi_case()
    M = blocks_cases.MULTI
    yield "multi", (ref, ctgs), dict(minctglength=blocks_cases.MULTI_MINCTG, mincluster=M["minclustsize"], minlength=M["minlength"], cluster=M["cluster"], maxdist=M["maxdist"])
    yield "1a+1brc", tuple(blocks_cases.fixture_inputs("1a+1brc")), dict(minctglength=100)


@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("pair", ["multi", "1a+1brc"])
def test_synteny_layout(pair, sa64, monkeypatch):
    t = transform()
    (ref, ctgs), kw = next((p[1], p[2]) for p in pairs() if p[0] == pair)
    tail = dict(minchainsum=30, greedy=False)
    chain = t.synteny_chain(ref, ctgs, sa64=sa64, **kw)
    want = t.chain_tail(chain["chain"], chain["rlength"], chain["qlength"], chain["ctg2range"], sa64=sa64, **tail)
    for below in ("shipped", 0):
        if below == 0:
            monkeypatch.setenv("RV_MERGE_HOST_BELOW", "0")                      # the kernels inside the pipeline
        got = t.synteny_layout(ref, ctgs, sa64=sa64, **kw, **tail)
        for k in ("blocks", "weight", "cost", "edgecosts", "extended"):
            assert got[k] == want[k], k
        for k in ("ctg2range", "rlength", "qlength", "sep", "refnames", "ctgnames", "mums"):
            assert got[k] == chain[k], k
        assert got["info"]["blocks"] == len(chain["blocks"]) and got["info"]["merge"]["rows_in"] == len(chain["chain"]) >= 2
        assert got["info"]["merge"]["rows_out"] == len(want["info"]["stages"]["merged"]) and got["info"]["stages"] == want["info"]["stages"]
        assert got["info"]["glocal"]["after"] == chain["info"]["after"] and got["info"]["sweeps"] == want["info"]["sweeps"]
        if below == 0:
            assert got["info"]["merge"]["route"] == "device" and got["info"]["merge"]["bytes_up"] == ROW * len(chain["blocks"]) + 4 * len(chain["chain"])
    assert len(want["blocks"]) >= 1 and len(want["extended"]) == len(want["blocks"])
