"""The capacity protocols (DESIGN.md "Lists filled by atomics") at small shapes: every list a kernel fills by atomics behind an estimated
capacity is overflowed on purpose -- by a dense input of tests/dense_cases.py where a small one exists, through RV_CAP_LIMIT / RV_CAP_SITES
where none does -- so that the driver's retry, or the anchor cascade's give-up and the level pipeline's rerun, is what produces the result.
Every case: the result equals the CPU oracle's; the counter of the retry (idx.capacity_events()) or the cascade's `why` shows that the
protocol ran; a second run on the same handle after reset() gives the same result."""
import functools
import os
import sys

import numpy as np
import pytest

import dense_cases as dc
from helpers import ROOT, assemble, csr_tuples, feed, oracle, rem, synth

sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu
MINL = dc.MINL
FIELDS = ("key", "n", "depth", "nsamples", "nnodes", "nmums", "picked", "l", "mn", "sp_min", "h_sa", "h_lcp", "h_mums")
SITE = {"multi_cand": 1, "cas_wit": 2, "cas_tables": 4, "casm_matches": 8, "casm_wit": 16, "casm_tables": 32, "mems_rec": 64, "mems_mem": 128, "mems_long": 256}


def mod(sa64):
    from reveal_amd import reveallib, reveallib64
    return reveallib64 if sa64 else reveallib


def aset(a):
    if len(a) == 4:
        l, n, off, pos = a
    else:
        l, off, pos = a
    return sorted((int(l[k]), tuple(int(x) for x in pos[off[k]:off[k + 1]])) for k in range(len(l)))


def digest(tr):
    o = np.lexsort((tr["key"], tr["depth"]))
    return {f: tr[f][o].astype(np.uint64) for f in FIELDS}


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name == "related_pair":
        return [g.decode() for g in synth.genomes(100000, 2)]
    if name == "related_triple":
        return [g.decode() for g in synth.genomes(60000, 3)]
    if name == "small_repetitive_triple":
        return dc.repetitive_triple(2000, 31, 40)
    if name == "tiny_repetitive_triple":
        return dc.repetitive_triple(600, 31, 12)
    if name == "large_undecided":
        from test_gpu_cascade import large_undecided_input
        return large_undecided_input()
    return getattr(dc, name)()


@functools.lru_cache(maxsize=None)
def reference(name, minl, minn=2, sa64=False):
    """the oracle's literal recursion, computed once per input: sorted anchors, final text, trace digest"""
    seqs = inputs(name)
    T, nsep, nodes = assemble(seqs)
    O = oracle(sa64)
    c = O.construct(T, nsep, len(seqs))
    ref = O.align_bench(c, nodes, minl, minn, trace_cap=4 * len(T) // max(minl, 1) + 1000)
    return dict(anchors=aset(ref["anchors"]), T=ref["T"], trace=digest(ref["trace"]), text=T)


def builtin(name, minl, minn=2, sa64=False, trace=False, opts=None):
    """align_builtin on a fresh handle with the switches `opts`, then once more after reset(): both results equal the oracle's.
    -> (capacity_events, cascade_info) of the first run"""
    seqs, ref = inputs(name), reference(name, minl, minn, sa64)
    idx = mod(sa64).index()
    for k, v in (opts or {}).items():
        idx.set_option(k, v)
    first = None
    for turn in range(2):
        if turn:
            idx.reset()
        feed(idx, seqs)
        idx.construct()
        got = idx.align_builtin(minl, minn, trace=trace)
        assert aset(got["anchors"]) == ref["anchors"], (turn, idx.cascade_info())
        assert idx.T.encode("latin-1") == ref["T"], turn
        if trace:
            gd = digest(got["trace"])
            for f in FIELDS:
                assert len(gd[f]) == len(ref["trace"][f]) and (gd[f] == ref["trace"][f]).all(), (turn, f)
        if first is None:
            first = (idx.capacity_events(), idx.cascade_info())
        del got
    return first


def callbacks(name, minl, minn=2, sa64=False, opts=None, preselect=0):
    """index.align with the Python forms of the built-in callbacks: the picks are the oracle's anchors, the text its text; twice on one handle"""
    seqs, ref = inputs(name), reference(name, minl, minn, sa64)
    idx = mod(sa64).index()
    for k, v in (opts or {}).items():
        idx.set_option(k, v)
    first = None
    for turn in range(2):
        if turn:
            idx.reset()
        feed(idx, seqs)
        idx.construct()
        if preselect:
            idx.preselect(preselect)
        picks = []

        def pick(mums, sub, precomputed=False, minlength=0):
            r = rem.bench_mumpicker(mums, sub, precomputed=precomputed, minlength=minlength)
            if r:
                picks.append((int(r[0][0]), tuple(sorted(int(p) for _, p in r[0][2]))))
            return r
        idx.align(pick, rem.linear_graphalign, minl=minl, minn=minn)
        assert sorted(picks) == ref["anchors"], turn
        assert idx.T.encode("latin-1") == ref["T"], turn
        if first is None:
            first = idx.capacity_events()
    return first


# ---- the pair scan's two lists ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sa64", [False, True])
def test_getmums_on_a_fresh_handle_grows_both_lists(sa64):
    """level 0, compaction branch: 5 106 records beyond the tiles' slots against an overflow buffer of 4 624, 6 050 MUMs against an output list of 4 623"""
    seqs = inputs("unrelated_pair")
    T, nsep, nodes = assemble(seqs)
    O = oracle(sa64)
    c = O.construct(T, nsep, 2)
    l, a, b = O.getmums(c["tbuf"], c["SA"], c["LCP"], nsep, MINL)
    want = [(int(l[k]), (int(a[k]), int(b[k])), 0) for k in range(len(l))]
    idx = mod(sa64).index()
    for turn in range(2):
        if turn:
            idx.reset()
        feed(idx, seqs)
        idx.construct()
        assert idx.getmums(MINL) == want, turn
        if turn == 0:
            ev = idx.capacity_events()
            assert ev["pair_ovf"] >= 1 and ev["pair_out"] >= 1, ev
        else:
            assert idx.capacity_events()["pair_ovf"] == 0       # (the lists have grown: no second retry; construct() zeroed the counters)


@pytest.mark.parametrize("sa64", [False, True])
def test_cascade_scan_loop_grows_its_lists(sa64):
    """the anchor cascade's own copy of the scan loop (rv_cascade.hip), witness regions switched on: it is the first scan of a default run"""
    ev, info = builtin("unrelated_pair", MINL, sa64=sa64)
    assert ev["pair_ovf"] >= 1 or ev["pair_out"] >= 1, ev
    assert info["matches"] == 6050, info          # counted in the cascade's driver: its loop ended with the whole list (the level pipeline's scan finds the lists grown)


@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("more", [{}, {"RV_NO_EARLY_SPLIT": 1}, {"RV_NO_LEAF": 1}])
def test_picker_retry_behind_the_level_hook(more, sa64):
    """untraced level pipeline, level 1 of copies_pair: the picker branch finds the overflow buffer too small after the level's hook has queued the
    early split (and the leaf launch) against incomplete picks; k_decide must have decided nothing, and the hook runs again after the retry"""
    ev, info = builtin("copies_pair", MINL, sa64=sa64, opts=dict({"RV_NO_CASCADE": 1}, **more))
    assert ev["pair_pick_ovf"] >= 1, ev
    assert not info["done"]


@pytest.mark.parametrize("sa64", [False, True])
def test_compaction_retry_and_second_copy_at_level_one(sa64):
    """traced run: both lists overflow at level 1 (12 229 records), and the records of the retry do not fit the host copy level 0 sized (65)"""
    ev, info = builtin("copies_pair", MINL, sa64=sa64, trace=True)
    assert ev["pair_ovf"] >= 1 and ev["pair_out"] >= 1 and ev["pair_second_copy"] >= 1, ev


@pytest.mark.parametrize("sa64", [False, True])
def test_compaction_retry_under_python_callbacks(sa64):
    ev = callbacks("copies_pair", MINL, sa64=sa64)
    assert ev["pair_ovf"] >= 1 and ev["pair_out"] >= 1 and ev["pair_second_copy"] >= 1, ev


@pytest.mark.parametrize("sa64", [False, True])
def test_device_preselection_after_a_retry(sa64, capfd):
    """rv_set_preselect: level 1's 12 229 records are capped on the device (pair_topk) by the attempt that follows the retry -- they never reach the
    host, which RV_PRESEL_LOG's count of copied records shows beside the same run with the host doing the capping"""
    def copied():
        n = [int(line.split()[1]) for line in capfd.readouterr().err.splitlines() if line.startswith("preselect: ")]
        assert len(n) >= 2, n      # (a line per alignment: the run and its repeat after reset())
        return n
    ev = callbacks("copies_pair", MINL, sa64=sa64, opts={"RV_PRESEL_DEV_MIN": 1000, "RV_PRESEL_LOG": 1}, preselect=100)
    assert ev["pair_ovf"] >= 1 or ev["pair_out"] >= 1, ev
    dev = copied()
    callbacks("copies_pair", MINL, sa64=sa64, opts={"RV_PRESEL_DEV_MIN": 1 << 40, "RV_PRESEL_LOG": 1}, preselect=100)
    host = copied()
    # level 1 alone: 12 229 records copied by the one, 100 per sub-index at most by the other (and levels 2, 3, ... save more)
    assert len(dev) == len(host) and sum(dev) + 2 * (12229 - 2 * 100) <= sum(host), (dev, host)


@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("trace", [False, True])
def test_fresh_worker_takes_a_dense_frontier(trace, sa64):
    """frontier hand-off (reveal_amd/shard.py) at level 1: a handle that has never scanned anything imports one of the two dense sub-indices;
    then the same once more on the same two handles after reset()"""
    seqs = inputs("copies_pair")
    M = mod(sa64)
    owner, w = M.index(), M.index()
    for idx in (owner, w):
        idx.set_option("RV_NO_CASCADE", 1)       # (the cascade would finish the run before there is a frontier to divide)
    for turn in range(2):
        if turn:
            owner.reset(); w.reset()
        ev = _divided_once(owner, w, seqs, trace, reference("copies_pair", MINL, 2, sa64))
        if turn:
            continue
        if trace:
            assert ev["pair_ovf"] >= 1 and ev["pair_out"] >= 1, ev
        else:
            assert ev["pair_pick_ovf"] >= 1, ev


def _divided_once(owner, w, seqs, trace, ref):
    from reveal_amd import shard
    feed(owner, seqs)
    feed(w, seqs)
    owner.construct()
    lib = owner._lib
    assert owner.align_builtin_until(2, MINL, 2, trace=trace) == 2
    fr = owner.frontier()
    packed = []
    for subs in shard.partition(fr["meta"][:, 1], 2):
        part = shard.subset(fr, subs)
        m = int(part["meta"][:, 1].sum())
        bufs = (np.zeros(max(m, 1), lib.sa_t), np.zeros(max(m, 1), lib.lcp_t), np.zeros(max(m, 1), np.uint8))
        owner.frontier_pack(subs, *bufs)
        packed.append((part, bufs))
    assert all(len(p["meta"]) == 1 for p, _ in packed)
    owner.frontier_import(packed[0][0], *packed[0][1], minl=MINL, minn=2)
    w.frontier_import(packed[1][0], *packed[1][1], minl=MINL, minn=2, maxlcp=owner.maxlcp, trace=trace)
    res = [owner.align_builtin_resume(), w.align_builtin_resume()]
    ev = w.capacity_events()
    got = shard.merge(res)
    assert aset(got["anchors"]) == ref["anchors"]
    assert shard.lower_text(ref["text"], got["anchors"]).tobytes() == ref["T"]
    if trace:
        gd = digest(got["trace"])
        for f in FIELDS:
            assert len(gd[f]) == len(ref["trace"][f]) and (gd[f] == ref["trace"][f]).all(), f
    return ev


# ---- more than two samples -------------------------------------------------------------------------------------------------------------

def test_multi_scan_retry_at_level_one():
    """traced run of copies_triple: 11 340 records with 22 680 members and more at level 1, against lists of 4 624 and 10 379"""
    ev, info = builtin("copies_triple", MINL, 2, trace=True)
    assert ev["multi_rec"] >= 1 and ev["multi_mem"] >= 1, ev


def test_multi_scan_retry_under_python_callbacks():
    ev = callbacks("copies_triple", MINL, 2)
    assert ev["multi_rec"] >= 1 and ev["multi_mem"] >= 1, ev


@pytest.mark.parametrize("minn", [2, 3])
@pytest.mark.parametrize("more", [{}, {"RV_NO_EARLY_SPLIT": 1}])
def test_multi_picker_redo(minn, more):
    """the picker's candidate list limited to one entry per region: the early split (k_decide_multi) sees the overflow and decides nothing,
    the picks are computed again and the commit splits (`redo`, rv_align.hip)"""
    opts = dict({"RV_NO_CASCADE": 1, "RV_CAP_LIMIT": 64, "RV_CAP_SITES": SITE["multi_cand"]}, **more)
    ev, info = builtin("copies_triple", MINL, minn, opts=opts)
    assert ev["multi_cand"] >= 1, ev


@pytest.mark.parametrize("name,minl", [("copies_triple", MINL), ("small_repetitive_triple", MINL), ("tiny_repetitive_triple", 1)])
def test_getmultimems_regrows_its_three_lists(name, minl):
    seqs = inputs(name)
    T, nsep, nodes = assemble(seqs)
    O = oracle(False)
    c = O.construct(T, nsep, len(seqs))
    want = csr_tuples(*O.getmultimums(c["tbuf"], c["SA"], c["LCP"], c["SO"], nsep, len(seqs), minl, 2, mems=True))
    idx = mod(False).index()
    idx.set_option("RV_CAP_LIMIT", 1)
    idx.set_option("RV_CAP_SITES", SITE["mems_rec"] | SITE["mems_mem"] | SITE["mems_long"])
    for turn in range(2):
        if turn:
            idx.reset()
        feed(idx, seqs)
        idx.construct()
        assert idx.getmultimems(minl, 2) == want, turn
        ev = idx.capacity_events()
        assert ev["mems_rec"] >= 1 and ev["mems_mem"] >= 1, ev
        if name == "small_repetitive_triple":       # (runs that nest 25 deep: tests/test_cpu_dense_cases.py; random text has none)
            assert ev["mems_long"] >= 1, ev


# ---- the cascades' give-ups --------------------------------------------------------------------------------------------------------------

PAIR_GIVE_UPS = [
    ("tandem_pair", 20, {"RV_CAP_LIMIT": 1, "RV_CAP_SITES": SITE["cas_wit"]}, "too many repeat witnesses"),
    # (a batch of one level: anchors of the finished levels have left for the host before the table fills up)
    ("related_pair", 20, {"RV_CAP_LIMIT": 64, "RV_CAP_SITES": SITE["cas_tables"], "RV_CASCADE_BATCH": 1}, "the cascade's tables are full"),
    ("contig_pair", 20, {"RV_CAP_LIMIT": 1, "RV_CAP_SITES": SITE["cas_tables"]}, "more sequences than the cascade's tables hold"),
]
MULTI_GIVE_UPS = [
    ("related_triple", 20, {"RV_CAP_LIMIT": 64, "RV_CAP_SITES": SITE["casm_matches"]}, "more full matches than the list holds"),
    ("repetitive_triple", 20, {"RV_CAP_LIMIT": 1, "RV_CAP_SITES": SITE["casm_wit"]}, "too many repeat witnesses"),
    ("related_triple", 20, {"RV_CAP_LIMIT": 1, "RV_CAP_SITES": SITE["casm_tables"]}, "tables are full"),
    ("large_undecided", 20, {"RV_CASM_BIG_ROOT": 9000}, "above the size that is rebuilt from the text"),
    ("large_undecided", 20, {"RV_CASM_BIG_TOTAL": 20000}, "above the size that is rebuilt from the text"),
]


@pytest.mark.parametrize("name,minl,opts,why", PAIR_GIVE_UPS + MULTI_GIVE_UPS)
def test_cascade_gives_up_and_the_level_pipeline_finishes(name, minl, opts, why):
    ev, info = builtin(name, minl, opts=opts)
    assert not info["done"] and why in info["why"], info
    if "RV_CAP_LIMIT" in opts and name in ("related_pair", "related_triple"):      # without the limit the cascade does these runs: what gave up is the list named
        assert builtin(name, minl)[1]["done"]


@pytest.mark.parametrize("name,minl,opts,why", [PAIR_GIVE_UPS[1], MULTI_GIVE_UPS[2]])
def test_give_up_with_the_callers_arrays(name, minl, opts, why):
    """rv_set_result_buffers: the abandoned attempt may have copied anchors ahead into the caller's arrays; what the run delivers is the
    oracle's anchors and nothing behind their count"""
    from reveal_amd._index import _page_array
    seqs, ref = inputs(name), reference(name, minl)
    na, nm = len(ref["anchors"]), sum(len(p) for _, p in ref["anchors"])
    idx = feed(mod(False).index(), seqs)
    for o, v in opts.items():
        idx.set_option(o, v)
    for turn in range(2):
        if turn:
            idx.reset()
            feed(idx, seqs)
        idx._dll.rv_set_result_buffers(idx._h, None, 0, None, 0, None, 0)       # (arrays are cleared before they are freed: include/reveal_amd.h)
        idx.__dict__.pop("_res_bufs", None)
        room = 64
        l, off, pos = _page_array(na + room, np.uint32), _page_array(na + 1 + room, np.int64), _page_array(nm + room, np.int64)
        l[:] = 0xFFFFFFFF; off[:] = -1; pos[:] = -1
        idx.__dict__["_res_bufs"] = (l, off, pos)       # (what align_builtin offers the library when nobody else holds them)
        del l, off, pos
        idx.construct()
        got = idx.align_builtin(minl, 2)
        info = idx.cascade_info()
        assert not info["done"] and why in info["why"], info
        assert aset(got["anchors"]) == ref["anchors"], turn
        gl, goff, gpos = got["anchors"]
        l, off, pos = idx.__dict__["_res_bufs"]
        assert gl.ctypes.data == l.ctypes.data and gpos.ctypes.data == pos.ctypes.data       # the caller's arrays are what came back
        assert len(gl) == na and (l[na:] == 0xFFFFFFFF).all() and (off[na + 1:] == -1).all() and (pos[nm:] == -1).all()
        del got, gl, goff, gpos, l, off, pos


# ---- the soak's generator with the limit on every site ----------------------------------------------------------------------------------

def test_fuzz_with_limited_capacities():
    """two cases of tools/fuzz.py (the same generator as tests/test_gpu_fuzz.py, a fixed number of cases instead of a time budget) under the
    RV_CAP_LIMIT entry of its ENVS alone: every estimate that RV_CAP_LIMIT reaches starts at 48"""
    import subprocess
    from fuzz import ENVS
    entry = [k for k, e in enumerate(ENVS) if "RV_CAP_LIMIT" in e]
    assert len(entry) == 1
    env = {k: v for k, v in os.environ.items() if not k.startswith("RV_")}
    env.update(FUZZ_CASES="2", FUZZ_ENVS=str(entry[0]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz.py"), "3600", "4"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "fuzz: 2 cases x (1 configurations" in r.stdout and "identical to the oracle" in r.stdout
