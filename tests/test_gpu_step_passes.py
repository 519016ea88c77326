"""Passes a construct() + align_builtin() step no longer makes: the radix sort's first histogram counts the digit bytes k_init_keys
leaves beside the keys (rv_radix_first_digits) instead of reading the keys back, and the working copy of the text is made when something
first needs it (rv_ensure_working_text) instead of in front of the SA build.  Results are the oracle's either way."""
import functools

import numpy as np
import pytest

from helpers import assemble, csr_tuples, feed, oracle, synth

pytestmark = pytest.mark.gpu


def mod(sa64):
    from reveal_amd import reveallib, reveallib64
    return reveallib64 if sa64 else reveallib


def aset(a):
    l, off, pos = a[0], a[-2], a[-1]
    return sorted((int(l[k]), tuple(int(x) for x in pos[off[k]:off[k + 1]])) for k in range(len(l)))


@functools.lru_cache(maxsize=None)
def inputs_of(length, k, seed):
    return tuple(g.decode() for g in synth.genomes(length, k, seed=seed))


@functools.lru_cache(maxsize=None)
def reference(length, k, seed, sa64=False):
    """the oracle's index of synth.genomes(length, k), made once: (T, SA, LCP, the top-level scan's matches: pairs for two samples,
    multi-sample matches otherwise)"""
    T, nsep, nodes = assemble(list(inputs_of(length, k, seed)))
    O = oracle(sa64)
    c = O.construct(T, nsep, k)
    if k == 2:
        l, a, b = O.getmums(c["tbuf"], c["SA"], c["LCP"], nsep, 20)
        mums = [(int(l[j]), (int(a[j]), int(b[j])), 0) for j in range(len(l))]
    else:
        mums = csr_tuples(*O.getmultimums(c["tbuf"], c["SA"], c["LCP"], c["SO"], nsep, k, 20, k))
    return T, c["SA"].copy(), c["LCP"].copy(), mums


def check_index(length, k, seed=3, sa64=False, byte_path=None):
    """SA and LCP against the oracle's.  The index hands out no BWT array: its bytes (the character in front of every suffix, bit 7 the sample
    side) are checked through the scans that read them instead of SA and the text, match for match against the oracle's -- the pair scan for two
    samples, the multi-sample scan otherwise.  byte_path: whether the conditions under which k_init_keys leaves the first pass' digit bytes
    (rv_radix_first_digits: 2^20 keys or more in the sort, more than one pass, the switch unset) must hold / must not hold for this input"""
    T, SA, LCP, mums = reference(length, k, seed, sa64)
    idx = feed(mod(sa64).index(), list(inputs_of(length, k, seed)))
    idx.construct()
    assert np.array_equal(idx.array("SA"), SA), "SA differs from the oracle"
    assert np.array_equal(idx.array("LCP"), LCP), "LCP differs from the oracle"
    assert len(mums) > 100
    assert (idx.getmums(20) if k == 2 else idx.getmultimums(20, k)) == mums
    if byte_path is not None:
        st = idx.sa_stats()
        on = st["sorted_elems"] >= (1 << 20) and st["radix_passes"] > 1 and idx.get_option("RV_RS_NO_DIGIT_BYTES") == 0 and idx.get_option("RV_RS_BITS") != 10
        assert on == byte_path, st
    return idx


# ---- the first pass' digit bytes (the byte path is on from 2^20 keys)

@pytest.mark.parametrize("sa64", [False, True])
def test_first_digits_from_init_keys_two_samples(sa64):
    """2 x 1 Mbp, related: the second sample's twins leave before the sort, about 1.17 x 10^6 keys stay -- above 2^20: the vector stores of the
    first sample's tiles, the byte stores of the kept suffixes and of the tile the second sample starts in"""
    idx = check_index(1_000_000, 2, sa64=sa64, byte_path=True)
    assert idx.sa_stats()["sorted_elems"] < idx.n      # (twins did leave: the kept-suffix path wrote digits)


def test_first_digits_without_twin_collapse(monkeypatch):
    monkeypatch.setenv("RV_NO_TWIN_COLLAPSE", "1")      # every suffix stays in the sort: four keys and one digit word per thread throughout
    idx = check_index(1_000_000, 2, byte_path=True)
    assert idx.sa_stats()["sorted_elems"] >= idx.n


def test_first_digits_three_samples():
    check_index(400_000, 3, byte_path=True)      # (no collapse with more than two samples; 1.2 x 10^6 keys)


def test_digit_bytes_switched_off(monkeypatch):
    monkeypatch.setenv("RV_RS_NO_DIGIT_BYTES", "1")     # the helper hands out no pointer: the first histogram reads the keys
    check_index(1_000_000, 2, byte_path=False)


def test_below_the_byte_path():
    check_index(200_000, 2, byte_path=False)      # 4 x 10^5 keys at most: below 2^20


# ---- the working text, made lazily

@functools.lru_cache(maxsize=None)
def _ref_run(length, seed, minl=20):
    """(the text as assembled, the oracle's run on it), made once.  (align_bench consumes the index it is given: one of its own)"""
    T, nsep, nodes = assemble(list(inputs_of(length, 2, seed)))
    O = oracle(False)
    return T, O.align_bench(O.construct(T, nsep, 2), nodes, minl, 2)


def test_text_after_construct_alone():
    T, ref = _ref_run(200_000, 3)
    idx = feed(mod(False).index(), list(inputs_of(200_000, 2, 3)))
    idx.construct()
    assert idx.T.encode("latin-1") == T      # the first reader makes the copy
    assert idx.T.encode("latin-1") == T


def test_text_after_two_constructs_and_align():
    T, ref = _ref_run(200_000, 3)
    idx = feed(mod(False).index(), list(inputs_of(200_000, 2, 3)))
    idx.construct()
    idx.construct()
    got = idx.align_builtin(20, 2)
    assert aset(got["anchors"]) == aset(ref["anchors"])
    assert idx.T.encode("latin-1") == ref["T"]
    idx.construct()      # a copy that is due again: the lower case of the run before is gone
    assert idx.T.encode("latin-1") == T
    got = idx.align_builtin(20, 2)
    assert aset(got["anchors"]) == aset(ref["anchors"]) and idx.T.encode("latin-1") == ref["T"]


def test_clone_between_construct_and_align():
    T, ref = _ref_run(200_000, 3)
    idx = feed(mod(False).index(), list(inputs_of(200_000, 2, 3)))
    idx.construct()
    cp = idx.copy()
    assert cp.T.encode("latin-1") == T
    got = idx.align_builtin(20, 2)
    assert aset(got["anchors"]) == aset(ref["anchors"]) and idx.T.encode("latin-1") == ref["T"]
    assert cp.T.encode("latin-1") == T      # its own text


def test_text_through_the_level_pipeline(monkeypatch):
    monkeypatch.setenv("RV_NO_CASCADE", "1")
    T, ref = _ref_run(200_000, 3)
    idx = feed(mod(False).index(), list(inputs_of(200_000, 2, 3)))
    idx.construct()
    got = idx.align_builtin(20, 2)
    assert not idx.cascade_info()["done"]
    assert aset(got["anchors"]) == aset(ref["anchors"])
    assert idx.T.encode("latin-1") == ref["T"]
