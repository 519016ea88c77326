"""construct(rc=1) with the reverse complement made in device memory (k_text_revcomp, csrc/rv_revcomp.hip) against the CPU oracle and against the
RV_RC_HOST leg (the host loop and a second upload), on the cases of tests/rc_cases.py, both libraries; the host text's lazy update behind every
reader and writer (rv_host_text); the counters of index.text_info(); getblocks, transform.synteny_blocks and align_builtin downstream.
The device leg is forced with RV_RC_HOST_BELOW = 0 wherever a test is about it, whatever the shipped threshold."""
import numpy as np
import pytest

import blocks_cases as BC
import rc_cases as C
from helpers import feed, oracle

pytestmark = pytest.mark.gpu

MINL = 10
SMALL = C.small_cases()
SMALL.update(C.fixture_cases())


def mod(sa64):
    from reveal_amd import reveallib, reveallib64
    return reveallib64 if sa64 else reveallib


def make(case, sa64, host=False, idx=None, **kw):
    """an index fed with the case, on the device leg (forced) or the host leg"""
    idx = feed(mod(sa64).index(**kw) if idx is None else idx, case, toupper=False)
    idx.set_option("RV_RC_HOST", 1 if host else 0)
    idx.set_option("RV_RC_HOST_BELOW", 0)
    return idx


def oracle_state(T, nsep, flips, rc, sa64, minl=MINL):
    """the text with its range reversed `flips` times, its SA, LCP and the MUMs as getmums gives them behind construct(rc)"""
    O = oracle(sa64)
    tb = O.textbuf(T)
    for _ in range(flips):
        O.revcomp(tb[nsep[0]:len(T)])
    SA = O.suffix_array(tb)
    LCP = O.compute_lcp(tb, SA, O.inverse(SA))
    l, a, b = O.getmums(tb, SA, LCP, nsep, minl, rc=rc, nT=len(T))
    return dict(T=tb[:len(T)].copy(), SA=SA, LCP=LCP, mums=[(int(l[k]), (int(a[k]), int(b[k])), rc) for k in range(len(l))])


def state(idx, minl=MINL):
    return dict(T=idx.array("T").copy(), SA=idx.array("SA").copy(), LCP=idx.array("LCP").copy(), mums=idx.getmums(minl))


def same(x, y, tag=None):
    for k in ("T", "SA", "LCP"):
        assert np.array_equal(x[k], y[k]), (k, tag)
    assert x["mums"] == y["mums"], ("mums", tag)


def guard_is_zero(idx):
    return not idx.text_guard().any()


# ---- 1. lengths, alphabet, shapes, fixtures; the alignment grid
@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("name", list(SMALL))
def test_cases_against_oracle_and_host_leg(name, sa64):
    case = SMALL[name]
    T, nsep, _ = C.text_of(case)
    dev = make(case, sa64)
    dev.construct(rc=0)
    dev.construct(rc=1)
    info = dev.text_info()
    assert (info["uploads"], info["rc_device"], info["rc_launches"]) == (1, 1, 1)
    assert guard_is_zero(dev)
    got = state(dev)
    same(got, oracle_state(T, nsep, 1, 1, sa64), name)
    host = make(case, sa64, host=True)
    host.construct(rc=0)
    host.construct(rc=1)
    same(got, state(host), name)
    assert np.array_equal(got["T"][:nsep[0]], np.frombuffer(T, dtype=np.uint8)[:nsep[0]])      # nothing in front of the range moved
    assert host.text_info()["rc_launches"] == 0


@pytest.mark.parametrize("sa64", [False, True])
def test_alignment_grid(sa64):
    """every lo mod 16 with every (lo + len) mod 16: 256 texts of under 200 bytes through two handles that are reset in between"""
    dev, host = mod(sa64).index(), mod(sa64).index()
    for r, c in C.ALIGNMENT_GRID:
        case = C.alignment_case(r, c)
        T, nsep, _ = C.text_of(case)
        assert nsep[0] == r and len(T) - nsep[0] == c + 2
        dev.reset(); host.reset()
        make(case, sa64, idx=dev); make(case, sa64, host=True, idx=host)
        for idx in (dev, host):
            idx.construct(rc=0)
            idx.construct(rc=1)
        assert dev.text_info()["rc_device"] == 1 and host.text_info()["rc_device"] == 0
        assert guard_is_zero(dev), (r, c)
        got = state(dev, 4)
        same(got, oracle_state(T, nsep, 1, 1, sa64, 4), (r, c))
        same(got, state(host, 4), (r, c))


def test_bytes_above_127_never_reach_the_device_text():
    """addsequence refuses them (bit 7 of a BWT byte carries the sample side), so the kernel never meets one; the rule leaves them unchanged
    (tests/test_cpu_rc.py)"""
    m = mod(False)
    idx = m.index()
    idx.addsample("a"); idx.addsequence(b"ACGT")
    idx.addsample("b")
    with pytest.raises(m.error, match="non-ASCII"):
        idx.addsequence(bytes(range(128, 256)))


# ---- 2. the point of the change
@pytest.mark.parametrize("sa64", [False, True])
def test_one_upload_and_a_host_text_that_owes_the_reversal(sa64):
    case = C.length_case(C.G + C.P + 1)
    T, nsep, _ = C.text_of(case)
    want = oracle_state(T, nsep, 1, 1, sa64)
    dev = make(case, sa64)
    dev.construct(rc=0)
    dev.construct(rc=1)
    info = dev.text_info()
    assert info == dict(uploads=1, upload_bytes=len(T), rc_device=1, host_stale=1, rc_launches=1)
    assert dev.T.encode("latin-1") == want["T"].tobytes()
    assert dev.text_info()["host_stale"] == 0
    assert dev.text_info()["uploads"] == 1
    host = make(case, sa64, host=True)
    host.construct(rc=0)
    host.construct(rc=1)
    info = host.text_info()
    assert info == dict(uploads=2, upload_bytes=2 * len(T), rc_device=0, host_stale=0, rc_launches=0)
    assert host.T == dev.T


# ---- 3. the first construct is the rc one
@pytest.mark.parametrize("sa64", [False, True])
def test_first_construct_is_rc(sa64):
    case = C.length_case(5 * C.G + 17)
    T, nsep, _ = C.text_of(case)
    dev = make(case, sa64)
    dev.construct(rc=1)
    info = dev.text_info()
    assert (info["uploads"], info["rc_device"], info["host_stale"]) == (1, 1, 1)
    host = make(case, sa64, host=True)
    host.construct(rc=1)
    assert host.text_info()["uploads"] == 1
    got = state(dev)
    same(got, state(host))
    same(got, oracle_state(T, nsep, 1, 1, sa64))


# ---- 4. twice
@pytest.mark.parametrize("sa64", [False, True])
def test_twice_owes_nothing(sa64):
    case = C.length_case(C.G + 1)
    T, nsep, _ = C.text_of(case)
    dev = make(case, sa64)
    dev.construct(rc=1)
    dev.construct(rc=1)
    info = dev.text_info()
    assert (info["uploads"], info["rc_device"], info["host_stale"], info["rc_launches"]) == (1, 1, 0, 2)      # the host was not touched
    host = make(case, sa64, host=True)
    host.construct(rc=1)
    host.construct(rc=1)
    got = state(dev)
    assert got["T"].tobytes() == T
    same(got, state(host))
    same(got, oracle_state(T, nsep, 2, 1, sa64))


def twice(case, sa64, times=2):
    """-> the two legs behind `times` construct(rc=1) calls"""
    out = []
    for host in (False, True):
        idx = make(case, sa64, host=host)
        for _ in range(times):
            idx.construct(rc=1)
        out.append(idx)
    return out


@pytest.mark.parametrize("sa64", [False, True])
def test_twice_on_bytes_the_rule_does_not_map_back(sa64):
    """U -> A -> T, u -> a -> t, ` -> @ -> @: two reversals of the alphabet case do not give the first text back, so the host owes both"""
    case = C.alphabet_case()
    T, nsep, _ = C.text_of(case)
    want = oracle_state(T, nsep, 2, 1, sa64)
    assert want["T"].tobytes() != T and len(want["T"]) == len(T)
    dev, host = twice(case, sa64)
    info = dev.text_info()
    assert (info["uploads"], info["host_stale"], info["rc_launches"]) == (1, 2, 2)
    got = state(dev)
    same(got, state(host))
    same(got, want)
    assert dev.text_info()["host_stale"] == 0
    # a third reversal on top of two owed ones equals one
    dev, host = twice(case, sa64, 3)
    assert dev.text_info()["host_stale"] == 1
    got = state(dev)
    same(got, state(host))
    same(got, oracle_state(T, nsep, 3, 1, sa64))
    same(got, oracle_state(T, nsep, 1, 1, sa64))
    # and a fourth two
    dev, host = twice(case, sa64, 4)
    assert dev.text_info()["host_stale"] == 2
    same(state(dev), state(host))


@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("what", ["addsequence", "copy", "upload_again"])
def test_state_after_two_reversals_of_such_bytes(what, sa64):
    """what reads or writes the host text behind two device reversals of the alphabet case finds the text the host leg and the oracle have"""
    case = C.alphabet_case()
    T, nsep, _ = C.text_of(case)
    legs = twice(case, sa64)
    assert legs[0].text_info()["host_stale"] == 2
    tb = oracle(sa64).textbuf(T)
    for _ in range(2):
        oracle(sa64).revcomp(tb[nsep[0]:len(T)])
    turned = tb[:len(T)].tobytes()
    if what == "addsequence":
        for idx in legs:
            idx.addsequence(b"ACGTTGCATTAGC")
            idx.construct()
        turned += b"ACGTTGCATTAGC$"
    elif what == "copy":
        legs = [idx.copy() for idx in legs]
        same(state(legs[0]), state(legs[1]))
        for c in legs:
            c.upload_again()
            c.construct(rc=0)
    else:
        for idx in legs:
            idx.upload_again()
            idx.construct(rc=0)
    assert legs[0].text_info()["host_stale"] == 0
    got = state(legs[0])
    same(got, state(legs[1]))
    assert got["T"].tobytes() == turned
    O = oracle(sa64)
    t2 = O.textbuf(turned)
    SA = O.suffix_array(t2)
    assert np.array_equal(got["SA"], SA) and np.array_equal(got["LCP"], O.compute_lcp(t2, SA, O.inverse(SA)))


# ---- 5. rc=1, then rc=0: the text stays reversed
@pytest.mark.parametrize("sa64", [False, True])
def test_rc_then_forward_keeps_the_reversed_text(sa64):
    case = C.shape_cases()["three_contigs_one_single_base"]
    T, nsep, _ = C.text_of(case)
    legs = []
    for host in (False, True):
        idx = make(case, sa64, host=host)
        idx.construct(rc=1)
        idx.construct(rc=0)
        legs.append(idx)
    assert legs[0].text_info()["host_stale"] == 1 and legs[0].text_info()["uploads"] == 1
    got = state(legs[0])
    same(got, state(legs[1]))
    same(got, oracle_state(T, nsep, 1, 0, sa64))


# ---- 6. the handle's state behind a device reversal
def both_legs(case, sa64, **kw):
    out = []
    for host in (False, True):
        idx = make(case, sa64, host=host, **kw)
        idx.construct(rc=0)
        idx.construct(rc=1)
        out.append(idx)
    assert out[0].text_info()["host_stale"] == 1
    return out


@pytest.mark.parametrize("sa64", [False, True])
def test_addsequence_after_a_device_reversal(sa64):
    case = C.length_case(2 * C.P + 1)
    T, nsep, _ = C.text_of(case)
    legs = both_legs(case, sa64)
    for idx in legs:
        idx.addsequence(b"ACGTTGCATTAGC")
        idx.construct()
    assert legs[0].text_info()["host_stale"] == 0 and legs[0].text_info()["uploads"] == 2
    got = state(legs[0], 4)
    same(got, state(legs[1], 4))
    tb = oracle(sa64).textbuf(T)
    oracle(sa64).revcomp(tb[nsep[0]:len(T)])
    assert got["T"].tobytes() == tb[:len(T)].tobytes() + b"ACGTTGCATTAGC$"


@pytest.mark.parametrize("sa64", [False, True])
def test_copy_after_a_device_reversal(sa64):
    case = C.length_case(C.G - 1)
    legs = both_legs(case, sa64)
    copies = [idx.copy() for idx in legs]
    same(state(copies[0]), state(copies[1]))
    same(state(copies[0]), state(legs[0]))
    for c in copies:                       # the copy's own host text: up it goes again, and the index is built from it
        c.upload_again()
        c.construct(rc=0)
    got = state(copies[0])
    same(got, state(copies[1]))
    T, nsep, _ = C.text_of(case)
    same(got, oracle_state(T, nsep, 1, 0, sa64))


@pytest.mark.parametrize("sa64", [False, True])
def test_upload_again_after_a_device_reversal(sa64):
    case = C.length_case(C.G)
    T, nsep, _ = C.text_of(case)
    legs = both_legs(case, sa64)
    for idx in legs:
        idx.upload_again()
        idx.construct(rc=0)
    assert legs[0].text_info()["host_stale"] == 0
    got = state(legs[0])
    same(got, state(legs[1]))
    same(got, oracle_state(T, nsep, 1, 0, sa64))


def test_cache_file_holds_the_reversed_text(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    case = C.fixture_cases()["1a+1brc"]
    T, nsep, _ = C.text_of(case)
    want = oracle_state(T, nsep, 1, 1, False)
    dev = make(case, False, cache=1)
    dev.construct(rc=1)
    assert (tmp_path / ".reveal.t").read_bytes() == want["T"].tobytes()
    assert dev.text_info()["rc_device"] == 1 and dev.text_info()["host_stale"] == 0
    assert np.array_equal(np.fromfile(str(tmp_path / ".reveal.sa"), dtype=np.int32), want["SA"])
    same(state(dev), want)


@pytest.mark.parametrize("sa64", [False, True])
def test_reset_after_a_device_reversal(sa64):
    legs = both_legs(C.length_case(C.G + 1), sa64)
    case = C.length_case(2 * C.P - 1, seed=5)
    T, nsep, _ = C.text_of(case)
    for k, idx in enumerate(legs):
        idx.reset()
        assert idx.text_info()["host_stale"] == 0
        make(case, sa64, host=bool(k), idx=idx)
        idx.construct(rc=0)
    got = state(legs[0], 4)
    same(got, state(legs[1], 4))
    same(got, oracle_state(T, nsep, 0, 0, sa64, 4))


# ---- 7. the threshold
def test_host_below_threshold():
    case = C.length_case(C.G + 1)
    T, nsep, _ = C.text_of(case)
    length = len(T) - nsep[0]
    want = oracle_state(T, nsep, 1, 1, False)
    shipped = mod(False).index().get_option("RV_RC_HOST_BELOW")
    for below, device in ((length + 1, 0), (length, 1), (0, 1), (None, 0 if length < shipped else 1)):
        idx = feed(mod(False).index(), case, toupper=False)
        if below is not None:
            idx.set_option("RV_RC_HOST_BELOW", below)
        idx.construct(rc=0)
        idx.construct(rc=1)
        info = idx.text_info()
        assert (info["rc_device"], info["uploads"]) == (device, 1 if device else 2), below
        same(state(idx), want, below)


# ---- 8. downstream
@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("name", list(BC.FIXTURES))
def test_getblocks_after_a_device_reversal(name, sa64):
    legs = []
    for host in (False, True):
        idx = feed(mod(sa64).index(), BC.fixture_inputs(name))
        idx.set_option("RV_RC_HOST", 1 if host else 0)
        idx.set_option("RV_RC_HOST_BELOW", 0)
        idx.set_option("RV_BLOCKS_HOST_BELOW", 0)
        idx.construct(rc=0)
        idx.construct(rc=1)
        legs.append(idx)
    assert legs[0].text_info()["rc_device"] == 1 and legs[1].text_info()["rc_device"] == 0
    for vname in ("defaults", "nocluster", "minclust0"):
        p = BC.params(**BC.VARIANTS[vname])
        args = (p["minlength"], p["cluster"], p["maxdist"], p["minclustsize"])
        got = legs[0].getblocks(*args)
        assert got == legs[1].getblocks(*args), vname
        assert BC.matches_golden(got, BC.golden()["fixtures"]["%s|rc1|%s" % (name, vname)]), vname
        assert len(got) > 0 or (name, vname) == ("1a+1b", "defaults")      # (a forward pair: no reverse-complement cluster reaches the default minclustsize)
    assert legs[0].text_info()["host_stale"] == 1      # nothing on the way read the host text


@pytest.mark.parametrize("sa64", [False, True])
def test_synteny_blocks_uploads_once(sa64, monkeypatch):
    from reveal_amd import transform as t
    ref, ctgs = BC.multi_case()
    kw = dict(minctglength=BC.MULTI_MINCTG, mincluster=BC.MULTI["minclustsize"], sa64=sa64, **{k: BC.MULTI[k] for k in ("minlength", "cluster", "maxdist")})
    monkeypatch.setenv("RV_RC_HOST_BELOW", "0")
    monkeypatch.delenv("RV_RC_HOST", raising=False)
    dev = t.synteny_blocks(ref, ctgs, **kw)
    monkeypatch.setenv("RV_RC_HOST", "1")
    host = t.synteny_blocks(ref, ctgs, **kw)
    assert dev["blocks"] == host["blocks"] and {b[4] for b in dev["blocks"]} == {0, 1}
    assert dev["text"]["uploads"] == 1 and dev["text"]["rc_device"] == 1 and dev["text"]["host_stale"] == 1
    assert host["text"]["uploads"] == 2 and host["text"]["rc_device"] == 0


@pytest.mark.parametrize("sa64", [False, True])
def test_align_builtin_after_a_device_reversal(sa64):
    case = C.fixture_cases()["1a+1brc"]
    res = []
    for host in (False, True):
        idx = make(case, sa64, host=host)
        idx.construct(rc=1)
        r = idx.align_builtin(20, 2)
        l, off, pos = r["anchors"]
        anchors = sorted((int(l[k]), tuple(int(x) for x in pos[off[k]:off[k + 1]])) for k in range(len(l)))      # (the order anchors come in is not fixed)
        res.append((anchors, idx.T))
    assert len(res[0][0]) > 0
    assert res[0][0] == res[1][0], "anchors"
    assert res[0][1] == res[1][1], "final text"
