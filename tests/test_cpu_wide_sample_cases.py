"""tests/wide_sample_cases.py itself, by the CPU oracle alone: every pinned (k, seed) still gives a family in which the recursion meets what
tests/test_gpu_wide_samples.py is there to compare -- conditions (a) .. (i) -- so that an edit of the generator cannot quietly empty the GPU
tests (as `synth70` of test_gpu_align.py was: more than 64 samples, one sub-index, nothing picked)."""
import pytest

import wide_sample_cases as wc


def test_every_sample_count_is_pinned():
    assert tuple(sorted(wc.SEEDS)) == wc.K
    # either side of every switch on the sample count
    for lo, hi in ((8, 9), (15, 16), (16, 17), (32, 33), (64, 65), (254, 255), (255, 256), (257, 258)):
        assert any(k <= lo for k in wc.K) and hi in wc.K
    assert {16, 17, 32, 33, 64, 65, 254, 255, 256, 257, 258} <= set(wc.K)


@pytest.mark.parametrize("k", wc.K)
def test_family_shape(k):
    seqs = wc.family(k, wc.SEEDS[k])
    assert len(seqs) == k and seqs[-1] == seqs[0]
    assert seqs == wc.family(k, wc.SEEDS[k])                       # deterministic
    assert len(set(seqs)) > min(k // 4, 16)                              # ... and a family, not k copies
    assert len({len(s) for s in seqs}) >= 4                        # regions deleted in subsets, an insertion in a subset
    assert all("N" * wc.NRUN in s for s in seqs) or k >= 100       # (at 300 bases a deleted region may take the run with it)
    assert sum(len(s) + 1 for s in seqs) <= 140000                 # the switches depend on k, not on the size


@pytest.mark.parametrize("k", wc.K)
def test_conditions(k):
    """(a) at least 8 anchors; (b) an anchor on fewer than k members, and top-level multi-MUMs with n = k and with n < k; (c) k >= 17: picks in
    sub-indices of <= 16 and of >= 17 samples; (d) k >= 33: an anchor of <= 16 members with one in a sample of id >= 32; (e) k >= 65: picks
    in sub-indices of <= 16 and of > 64 samples; (f) k >= 255: a pick in a sub-index of >= 255 samples; (g) at the root an LCP interval of
    exactly k ranks and a value of minlength and more in which a sample occurs twice, at ranks that are not neighbours; (h) two picked
    sub-indices of two samples and at most 64 ranks at one depth (side by side in one tile of the level: a candidate list of one entry per
    region overflows whatever k is); (i) k >= 17: an anchor of <= 16 members with samples 15 and 16 among them (the separator that is the last in
    a register and the first one loaded), k >= 33: one with samples 31 and 32 (either word of the census)"""
    ref = wc.reference(k, wc.SEEDS[k])
    figs = ref["figs"]
    print(figs)
    assert wc.missing(figs) == [], figs
    assert figs["ranks"] == len(ref["T"]) == len(ref["SA"])
    # the figures against the trace itself
    tr = ref["trace"]
    assert figs["subs"] == len(tr) == ref["steps"] and figs["picked"] == int(tr["picked"].sum()) == len(ref["anchors"]) == ref["splits"]
    assert int(tr["nsamples"].max()) == k and int(tr["nsamples"].min()) < k
    # an anchor has as many members as its sub-index has samples (the built-in picker takes matches on every sample only)
    assert sorted(len(p) for _, p in ref["anchors"]) == sorted(int(x) for x in tr["mn"][tr["picked"] != 0])
    assert all(int(x) == int(y) for x, y in zip(tr["mn"][tr["picked"] != 0], tr["nsamples"][tr["picked"] != 0]))
    # both top-level lists are there to be compared
    assert len(ref["mums"]) >= 100 and len(ref["mums_full"]) >= 8 and all(m[1] == k for m in ref["mums_full"])


def test_doubled_interval_count_on_a_known_text():
    """condition (g)'s counter on a text small enough to check by hand: three samples, a word of 14 bases once in the first and twice in
    the second, nowhere in the third"""
    from helpers import assemble, oracle
    w = "ACGTTGCATGCAGT"
    seqs = ["TT" + w + "CA", "GG" + w + "AG" + w + "TC", "CATCATCATCAT"]
    T, nsep, nodes = assemble(seqs)
    c = oracle(False).construct(T, nsep, 3)
    twice, apart = wc.doubled_root_intervals(c["SA"], c["LCP"], c["SO"], 3, minl=12)
    # the suffixes that begin 0, 1 and 2 bases into the word: three ranks each, in the order of what follows the word (AG.., CA$, TC$):
    # the second sample's two ranks have the first sample's between them
    assert (twice, apart) == (3, 3)
    assert wc.doubled_root_intervals(c["SA"], c["LCP"], c["SO"], 3, minl=len(w) + 1) == (0, 0)
    seqs[1] = "GG" + w + "CC" + w + "CG"      # (CA$, CC.., CG$: now they are neighbours, and the three share 15 bases: four intervals)
    T, nsep, nodes = assemble(seqs)
    c = oracle(False).construct(T, nsep, 3)
    assert wc.doubled_root_intervals(c["SA"], c["LCP"], c["SO"], 3, minl=12) == (4, 0)
