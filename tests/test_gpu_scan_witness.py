"""The anchor cascade's repeat witnesses come out of the top-level pair scan (k_scan_pair<true>, rv_scan.hip) and no longer from a pass of
their own over LCP and BWT (k_cas_witness, rv_cascade.hip; RV_CAS_WITNESS_PASS=1 brings it back).  The predicate is restated here in numpy
on the index' own SA and LCP: the count must be that of both settings, and everything a run hands out must be equal between them and equal
the oracle's.

The scan takes sixteen ranks per lane, 1024 per wave and 4096 per workgroup and fetches what lies around a wave from memory: the inputs are
chosen (seeds searched on the CPU with the oracle's arrays) so that expected witnesses sit on every one of these borders, at both ends of the
arrays and in a last wave that is only partly inside them -- test_inputs_cover_the_borders asserts that from the numpy lists."""
import functools
import random

import numpy as np
import pytest

from helpers import assemble, feed, oracle

MINL = 20
WAVE, GROUP = 1024, 4096


def mod(sa64):
    from reveal_amd import reveallib, reveallib64
    return reveallib64 if sa64 else reveallib


def aset(a):
    l, off, pos = a[0], a[-2], a[-1]
    return sorted((int(l[k]), tuple(int(x) for x in pos[off[k]:off[k + 1]])) for k in range(len(l)))


def make_inputs(length, seed, contigs=False, plain=False):
    """two samples of `length` bp: a random base and a copy with 1 % substitutions.  Unless plain: an interspersed repeat of minl characters
    and more, a tandem array with different point mutations in the two samples (the tandem cases of test_gpu_cascade_tail.py), a run of T
    (the largest suffixes: the last ranks of the arrays) and a run of A (the smallest
    ones that do not start with a separator: the first ranks a witness can have).  contigs: the first sample as two sequences"""
    rng = random.Random(seed)
    arr = ""
    if not plain:
        unit = "".join(rng.choice("ACGT") for _ in range(rng.choice([7, 23, 61])))
        arr = unit * (min(length // 3, rng.choice([600, 1500, 2500])) // len(unit))
        length -= len(arr)
    base = [rng.choice("ACGT") for _ in range(length)]
    if not plain:
        rep = [rng.choice("ACGT") for _ in range(rng.choice([25, 60, 150]))]
        for _ in range(rng.randint(4, 12)):
            p = rng.randint(0, length - 200)
            base[p:p + len(rep)] = rep
        p = rng.randint(0, length - 100)
        base[p:p + 60] = "T" * 60
        p = rng.randint(0, length - 100)
        base[p:p + 60] = "A" * 60
        base[-1] = "C"      # (no suffix "A$": the runs of A are the first ranks behind the separators')
    base = "".join(base)
    arr_a = arr_b = ""
    if not plain:
        def mutated(s, every):
            s = list(s)
            for q in range(rng.randint(0, every), len(s), every):
                s[q] = rng.choice("ACGT")
            return "".join(s)
        arr_a, arr_b = mutated(arr, 97), mutated(arr, 89)
    other = "".join(rng.choice("ACGT") if rng.random() < 0.01 else c for c in base)
    h = length // 2
    a, b = base[:h] + arr_a + base[h:], other[:h] + arr_b + other[h:]
    if contigs:
        cut = rng.randint(len(a) // 3, 2 * len(a) // 3)
        return [[b[:40] + a[40:cut], b[:40] + a[cut + 40:]], b]
    return [a, b]


# (length, seed, contigs): lengths that are no multiples of 1024 or 4096; the seeds make test_inputs_cover_the_borders hold
CASES = [(1500, 0, False), (3000, 0, True), (5200, 0, False), (8100, 2, False), (12000, 3, False)]
ZERO = (1500, 7)


def expected_witnesses(SA, LCP, nsep0, minl):
    """k_cas_witness' predicate (rv_cascade.hip): -> ranks, values.  Ranks outside the arrays count as LCP 0 and side 0"""
    n = len(SA)
    L = np.zeros(n + 3, dtype=np.int64)
    L[1:n + 1] = np.asarray(LCP).astype(np.int64)
    s = np.zeros(n + 2, dtype=np.int64)
    s[1:n + 1] = np.asarray(SA).astype(np.int64) > nsep0
    j = np.arange(n)
    lm1, l0, l1, l2 = L[j], L[j + 1], L[j + 2], L[j + 3]
    sm1, s0, s1 = s[j], s[j + 1], s[j + 2]
    pair0 = (j >= 1) & (l0 > lm1) & (l0 > l1) & (s0 != sm1)
    pair1 = (j + 1 < n) & (l1 > l0) & (l1 > l2) & (s1 != s0)
    w = np.where(pair0, np.maximum(lm1, l1), np.where(pair1, np.maximum(l0, l2), np.maximum(l0, l1)))
    hit = w >= minl
    return j[hit], w[hit]


@functools.lru_cache(maxsize=None)
def reference(length, seed, contigs=False, plain=False, sa64=False):
    """computed once per input and width, shared by the tests below"""
    inputs = make_inputs(length, seed, contigs, plain)
    T, nsep, nodes = assemble(inputs)
    O = oracle(sa64)
    c = O.construct(T, nsep, 2)
    ranks, _ = expected_witnesses(c["SA"], c["LCP"], nsep[0], MINL)
    ref = O.align_bench(c, nodes, MINL, 2)
    return dict(inputs=inputs, n=len(T), nseps=T.count(b"$"), nsep0=nsep[0], ranks=ranks, anchors=aset(ref["anchors"]), T=ref["T"], stats=ref["stats"])


def test_inputs_cover_the_borders():
    """(needs no GPU.)  Expected witnesses at ranks 1023, 0 and 1 mod 1024 (a wave's ends and what the next wave's first lane sees of them),
    4095 and 0 mod 4096 (a workgroup's), at ranks n - 2 and n - 1, at the first rank that can be one, and inside a last wave that is only partly
    inside the arrays.  Rank 1 itself cannot be a witness on any input: the suffixes that start with a separator come first, one rank each, with LCP 0
    (a separator matches nothing), and the LCP of the rank behind them is 0 as well -- with two separators or more the predicate sees nothing
    but zeros at rank 1, and at every separator's rank (asserted below).  The first rank that can be one is the smallest ordinary suffix', in
    the first wave's first lane: the runs of A put witnesses there"""
    seen = set()
    for length, seed, contigs in CASES:
        r = reference(length, seed, contigs)
        n, ranks = r["n"], r["ranks"]
        assert n > 2048 and n % WAVE and n % GROUP, n
        inner = ranks[ranks >= WAVE]      # (the borders between waves, not the arrays' first ranks)
        for m in (WAVE - 1, 0, 1):
            if (inner % WAVE == m).any():
                seen.add("wave %d" % m)
        for m in (GROUP - 1, 0):
            if (inner % GROUP == m).any():
                seen.add("group %d" % m)
        assert not (ranks < r["nseps"]).any()
        for name, rank in (("first", r["nseps"]), ("last but one", n - 2), ("last", n - 1)):
            if (ranks == rank).any():
                seen.add(name)
        if (ranks >= n - n % WAVE).any():
            seen.add("partial wave")
    assert seen == {"wave 1023", "wave 0", "wave 1", "group 4095", "group 0", "first", "last but one", "last", "partial wave"}, seen
    z = reference(ZERO[0], ZERO[1], plain=True)
    assert len(z["ranks"]) == 0 and z["n"] > 2048


def run(r, sa64, monkeypatch, witness_pass):
    if witness_pass:
        monkeypatch.setenv("RV_CAS_WITNESS_PASS", "1")
    else:
        monkeypatch.delenv("RV_CAS_WITNESS_PASS", raising=False)
    idx = feed(mod(sa64).index(), r["inputs"])
    idx.construct()
    ranks, _ = expected_witnesses(idx.array("SA"), idx.array("LCP"), r["nsep0"], MINL)
    got = idx.align_builtin(MINL, 2)
    info = idx.cascade_info()
    out = dict(anchors=aset(got["anchors"]), T=idx.T.encode("latin-1"), stats=dict(got["stats"]), info=info)
    print("n %d  expected witnesses %d  reported %d (RV_CAS_WITNESS_PASS=%d)  %s" % (r["n"], len(ranks), info["witnesses"], int(witness_pass), info))
    assert np.array_equal(ranks, r["ranks"])
    assert info["matches"] > 0, info      # (the cascade ran)
    assert info["witnesses"] == len(ranks), (info, len(ranks))
    assert out["anchors"] == r["anchors"]
    assert out["T"] == r["T"]
    st, rs = out["stats"], r["stats"]
    assert st["splits"] == rs["nsplits"] and st["steps"] == rs["nsteps"] and st["anchored_bp"] == rs["anchored_bp"]
    return out


def both_settings(r, sa64, monkeypatch):
    a = run(r, sa64, monkeypatch, False)
    b = run(r, sa64, monkeypatch, True)
    assert a == b
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("length,seed,contigs", CASES)
def test_scan_lists_the_witnesses(monkeypatch, length, seed, contigs, sa64):
    both_settings(reference(length, seed, contigs, sa64=sa64), sa64, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("sa64", [False, True])
def test_second_attempt_walks_the_scans_list(monkeypatch, sa64):
    """RV_CASCADE_DANGER=2: undecided sub-indices are decided from the witnesses in rank order -- the scan's list is in another order
    than the separate pass' and has to come out of the sort the same"""
    monkeypatch.setenv("RV_CASCADE_DANGER", "2")
    decided = 0
    for length, seed, contigs in CASES[2:]:
        decided += both_settings(reference(length, seed, contigs, sa64=sa64), sa64, monkeypatch)["info"]["decided_from_witnesses"]
    assert decided > 0


@pytest.mark.gpu
@pytest.mark.parametrize("sa64", [False, True])
def test_no_witness_at_all(monkeypatch, sa64):
    r = reference(ZERO[0], ZERO[1], plain=True, sa64=sa64)
    assert len(r["ranks"]) == 0
    assert both_settings(r, sa64, monkeypatch)["info"]["witnesses"] == 0
