"""The ordinary multi-sample path -- construct, getmultimums, the level pipeline's scan -> pick -> split -> bubble under the built-in picker --
at 6 .. 258 samples, on either side of every place where its code switches on the NUMBER OF SAMPLES: the 15 separators
k_full_scan keeps in registers (16 / 17), its 16-lane row form (sub-indices of 16 / 17 samples), the second census word (sample ids 32 and up,
in sub-indices of <= 16 samples too), k_multi_pick1 and the quadratic census above 64 samples, its sample counts of 255 and more and its
separators beyond 257 in global memory, the cascade's limit of 16 samples, construct's first-key groups of 9 and of 65 homologues.
The families are those of tests/wide_sample_cases.py (tests/test_cpu_wide_sample_cases.py holds them to what they are there to contain);
every comparison is against the CPU oracle on the same input, computed once per family."""
import numpy as np
import pytest

import wide_sample_cases as wc
from helpers import feed
from test_gpu_align import compare, mod

pytestmark = pytest.mark.gpu

ALT_K = (16, 17, 33, 65, 257, 258)        # the alternative paths
SA64_K = (16, 17, 33, 65, 258)            # the 64-bit library's recursion
BOTH_K = (9, 64, 65, 258)                 # construct on both libraries
SITE_MULTI_CAND = 1                       # RV_CAP_SITES: the multi picker's candidate list
ALT = {
    "no_cascade": {"RV_NO_CASCADE": 1},
    "scan_v1": {"RV_SCAN_V1": 1},                         # k_multi_pick1 below 65 samples too
    "no_early_split": {"RV_NO_EARLY_SPLIT": 1},
    "cand_retry": {"RV_NO_CASCADE": 1, "RV_CAP_LIMIT": 64, "RV_CAP_SITES": SITE_MULTI_CAND},      # one candidate per region: the picks are computed again
}


def ref_of(k, sa64=False):
    return wc.reference(k, wc.SEEDS[k], sa64)


def index_of(k, sa64=False, opts=None):
    idx = mod(sa64).index()
    for name, v in (opts or {}).items():
        idx.set_option(name, v)
    feed(idx, ref_of(k, sa64)["seqs"])
    idx.construct()
    return idx


def untraced(k, sa64=False, opts=None):
    """align_builtin(trace=False) on a fresh handle: anchors, final text, splits and anchored_bp are the oracle's.  -> the index"""
    ref = ref_of(k, sa64)
    idx = index_of(k, sa64, opts)
    got = idx.align_builtin(wc.MINL, 2, trace=False)
    info = idx.cascade_info()
    ga = wc.aset(got["anchors"])
    assert len(ga) == len(ref["anchors"]), (len(ga), len(ref["anchors"]), info)
    assert ga == ref["anchors"], info
    assert idx.T.encode("latin-1") == ref["text"]
    assert got["stats"]["splits"] == ref["splits"]
    assert got["stats"]["anchored_bp"] == ref["anchored_bp"]
    return idx, info


@pytest.mark.parametrize("k,sa64", [(k, False) for k in wc.K] + [(k, True) for k in BOTH_K])
def test_construct(k, sa64):
    ref = ref_of(k, sa64)
    idx = index_of(k, sa64)
    assert np.array_equal(idx.array("SA"), ref["SA"])
    assert np.array_equal(idx.array("LCP"), ref["LCP"])


@pytest.mark.parametrize("k", wc.K)
def test_getmultimums(k):
    """the whole list, order included: every multi-MUM of 12 bases and more on two samples and more, and those of 4 bases and more on all k"""
    ref = ref_of(k)
    idx = index_of(k)
    for minl, minn, want in ((wc.MINL, 2, ref["mums"]), (wc.MINL_FULL, k, ref["mums_full"])):
        got = idx.getmultimums(minlength=minl, minn=minn)
        assert len(got) == len(want), (minl, minn)
        assert got == want, (minl, minn)


@pytest.mark.parametrize("k", wc.K)
def test_traced_recursion(k):
    """all 13 fields of every sub-index, the anchor set, the final text, splits and steps"""
    ref = ref_of(k)
    compare(ref["seqs"], wc.MINL, 2, ref=ref["run"])


@pytest.mark.parametrize("k", wc.K)
def test_untraced_recursion(k):
    """what index.align's callers and bench.py run: the multi-sample cascade up to 16 samples, the level pipeline beyond"""
    idx, info = untraced(k)
    print("wide k=%d: cascade_info %s" % (k, info))
    if k >= 17:
        assert not info["done"], info


@pytest.mark.parametrize("k", ALT_K)
@pytest.mark.parametrize("path", sorted(ALT))
def test_alternative_paths(path, k):
    idx, info = untraced(k, opts=ALT[path])
    if "RV_NO_CASCADE" in ALT[path] or k >= 17:
        assert not info["done"], info
    if path == "cand_retry":
        ev = idx.capacity_events()
        assert ev["multi_cand"] >= 1, ev


@pytest.mark.parametrize("k", SA64_K)
def test_traced_recursion_64bit(k):
    ref = ref_of(k, True)
    compare(ref["seqs"], wc.MINL, 2, sa64=True, ref=ref["run"])


@pytest.mark.parametrize("k", SA64_K)
def test_untraced_recursion_64bit(k):
    idx, info = untraced(k, sa64=True)
    if k >= 17:
        assert not info["done"], info
