"""align_many with the reference's default picker for pair jobs above 2048 ranks (RV_MANY_CHAIN_LARGE), without a device: the job list of the GPU tests and
its golden file (tests/golden/many_chain_large.json: `rem.align` on the reference's own index, tools/gen_many_chain_large_golden.py), the conditions that
make the file a test of the picker, the admission rule of the shared launches, and the argument errors that come before the library is asked for a device."""
import os
import sys

import pytest

import many_cases as mc
import many_chain_large_cases as cl
import many_large_cases as lc
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many, schemes

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))


def as_bytes(pair):
    return [s.upper().encode() for s in pair]


@pytest.fixture(scope="module")
def jobs():
    return cl.jobs()


@pytest.fixture(scope="module")
def golden():
    return cl.load_golden()


def test_cases_are_deterministic_and_within_their_ranges(jobs):
    assert jobs == cl.jobs()
    assert len(jobs) == cl.N_CLASS + cl.N_REARRANGED + cl.N_DIVERGENT + 3
    assert jobs[:cl.N_CLASS] == lc.large_class_jobs(2)
    assert [n for n, _ in cl.SETS] == ["default", "wpen4", "wscore3", "star-avg", "star-med", "minl10"]
    ranks = [len(a) + len(b) + 2 for _, (a, b) in jobs]
    for (cls, _), r in zip(jobs, ranks):
        if cls == "rearranged-large":
            assert 2100 <= r <= 9000
        elif cls == "divergent-large":
            assert 17002 <= r <= 20000
        elif cls in lc.CLASSES:
            assert lc.RANKS_MIN <= r <= lc.RANKS_MAX
    assert sum(c == "rearranged-large" for c, _ in jobs) == 30
    assert ranks[-3:] == [2049, 20000, 20000] and jobs[-1][1][0] == jobs[-1][1][1]
    assert len(cl.big_job()[0]) + len(cl.big_job()[1]) + 2 == 80002
    assert len(cl.fillers()) == many.CHAIN_LARGE_MIN - 1
    # every job is admitted under every set, and only with the switch
    for name, kw in cl.SETS:
        args = cl.picker_args(kw)
        for cls, pair in jobs:
            assert many.takes_shared_launch(as_bytes(pair), picker=args, chain_large=True, minlength=kw["minlength"]), (name, cls)
            assert not many.takes_shared_launch(as_bytes(pair), picker=args, chain=True, chain_multi=True, chain_wide=True, large=True, minlength=kw["minlength"]), (name, cls)
    # rem.align's defaults do not admit the job of 80 002 ranks (a seed could arise, --maxmums could bite); its own set does
    big = as_bytes(cl.big_job())
    assert not many.takes_shared_launch(big, picker=cl.picker_args(dict(minlength=20)), chain_large=True)
    assert many.takes_shared_launch(big, picker=cl.picker_args(cl.BIG_SET[1]), chain_large=True)


def test_golden_file_is_self_consistent(jobs, golden):
    """anchors of a job are disjoint and collinear on both sequences, lie inside them, and the upper-cased text lower-cased over them is the
    recorded final text"""
    todo = [(name, pair, golden[name][j]) for name, _ in cl.SETS for j, (_, pair) in enumerate(jobs)] + [("big", cl.big_job(), golden["big"][0])]
    for name, (a, b), (anchors, sha) in todo:
        text = bytearray((a.upper() + "$" + b.upper() + "$").encode())
        la = len(a)
        assert anchors == sorted(anchors)
        by_a = sorted(anchors, key=lambda x: x[1][0])
        for k, (l, (pa, pb)) in enumerate(by_a):
            assert l >= 1 and 0 <= pa and pa + l <= la and la + 1 <= pb and pb + l <= len(text) - 1, name
            assert text[pa:pa + l] == text[pb:pb + l], name
            if k:
                l0, (qa, qb) = by_a[k - 1]
                assert qa + l0 <= pa and qb + l0 <= pb, (name, "not disjoint and collinear")
        for l, (pa, pb) in anchors:
            text[pa:pa + l] = text[pa:pa + l].lower()
            text[pb:pb + l] = text[pb:pb + l].lower()
        assert cl.sha(bytes(text)) == sha, name
    assert len(golden["roots"]) == len(jobs) and len(golden["candidates"]) == len(jobs) + 1
    for j, r in enumerate(golden["roots"]):
        assert (r is None) == (not golden["default"][j][0]) and (r is None or r in golden["default"][j][0])


def test_the_fixture_tests_the_picker(jobs, golden):
    """conditions (a) - (d) of tools/gen_many_chain_large_golden.py, the candidate counts recomputed with the CPU oracle"""
    import gen_many_chain_large_golden as gen
    cand = [cl.root_candidates(pair, 20) for _, pair in jobs] + [cl.root_candidates(cl.big_job(), 20)]
    assert cand == golden["candidates"]
    names = [n for n, _ in cl.SETS]
    bad = gen.conditions(cl, jobs, [r[0] for r in golden["default"]], {n: [cl.digest(r[0]) for r in golden[n]] for n in names[1:]}, golden["roots"],
                         cand[:-1], cand[-1], lambda j: mc.oracle_job(as_bytes(jobs[j][1]), 20)[0])
    assert not bad, bad


def test_what_the_shared_launches_take_under_the_switch():
    rng = __import__("random").Random(5)
    a = mc.rnd(rng, 1024)
    b = mc.mutate(rng, a, 0.01)
    args = schemes.PickerArgs(maxmums=10000)
    on = dict(chain_large=True)
    pair = [a.encode(), b.encode()]                                                                                     # 2050 ranks
    assert not many.takes_shared_launch([pair[0][:1023], pair[1][:1023]], picker=args, **on)                            # 2048 ranks: RV_MANY_CHAIN's
    assert many.takes_shared_launch([pair[0][:1023], pair[1][:1023]], picker=args, chain=True, **on)
    assert many.takes_shared_launch([pair[0], pair[1][:1023]], picker=args, **on)                                       # 2049
    assert not many.takes_shared_launch([pair[0], pair[1][:1023]], picker=args, chain=True)                             # ... and not without the switch
    big = (mc.rnd(rng, 1 << 16)).encode()
    wide = schemes.PickerArgs(maxmums=1 << 20, seedsize=1 << 20)
    assert many.takes_shared_launch([big[:(1 << 16) - 1], big[:(1 << 16) - 1]], picker=wide, **on)                      # 2^17 ranks
    assert not many.takes_shared_launch([big, big[:(1 << 16) - 1]], picker=wide, **on)                                  # 2^17 + 1
    assert not many.takes_shared_launch([big, big], picker=wide, large_max=1 << 20, **on)                               # ... whatever RV_MANY_LARGE_MAX says
    assert not many.takes_shared_launch([big[:5000], big[:5000]], picker=wide, large_max=10000, **on)                   # ... which still bounds the class
    assert not many.takes_shared_launch(pair, picker=schemes.PickerArgs(maxmums=10000, trim=False), **on)
    assert not many.takes_shared_launch(pair, picker=args, minlength=0, **on)                                           # the p-value cut stays on the host
    assert not many.takes_shared_launch(pair, picker=schemes.PickerArgs(maxmums=10000, seedsize=30), **on)              # a seed could arise
    assert not many.takes_shared_launch(pair, picker=schemes.PickerArgs(maxmums=10000, seedsize=1024), **on)
    assert many.takes_shared_launch(pair, picker=schemes.PickerArgs(maxmums=10000, seedsize=1025), **on)
    assert many.takes_shared_launch(pair, picker=schemes.PickerArgs(maxmums=10000, seedsize=0), **on)
    assert not many.takes_shared_launch(pair, picker=schemes.PickerArgs(maxmums=10000, wpen=2000), **on)
    assert many.takes_shared_launch(pair, picker=schemes.PickerArgs(maxmums=10000, wpen=many.CHAIN_MULTI_WMAX, wscore=many.CHAIN_MULTI_WMAX), **on)
    assert not many.takes_shared_launch(pair, picker=schemes.PickerArgs(maxmums=10000, wscore=many.CHAIN_MULTI_WMAX + 1), **on)
    assert not many.takes_shared_launch(pair, picker=schemes.PickerArgs(maxmums=10000, wpen=-1), **on)
    assert not many.takes_shared_launch(pair, picker=schemes.PickerArgs(maxmums=1023), **on)                            # below the shorter sequence
    assert many.takes_shared_launch(pair, picker=schemes.PickerArgs(maxmums=1024), **on)
    assert not many.takes_shared_launch(pair + [pair[0]], picker=args, **on)                                            # three sequences
    assert not many.takes_shared_launch([pair[0], pair[1][:500] + b"\0" + pair[1][501:]], picker=args, **on)
    # no picker: the switch means nothing
    assert not many.takes_shared_launch(pair, **on) and many.takes_shared_launch(pair, large=True, **on)
    # rem.align's defaults: every bubble `reveal refine` takes (alleles below 10 000 bases), nothing with an allele of 10 000
    dflt = cl.picker_args(dict(minlength=20))
    assert many.takes_shared_launch([big[:9999], big[:9999]], picker=dflt, **on)
    assert not many.takes_shared_launch([big[:10000], big[:2000]], picker=dflt, **on)


@pytest.mark.parametrize("bad", [dict(maxdepth=3), dict(maxsize=100)])
def test_unsupported_picker_options_raise_before_any_device(bad, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(many, "Batch", no_device)
    job = [["ACGT" * 600, "ACGT" * 600]]
    with pytest.raises(many.error, match="maxbubblesize / maxdepth"):
        many.align_many(job, picker=schemes.PickerArgs(**bad), chain_large=True)
    with pytest.raises(many.error, match="gap cost model"):
        many.align_many(job, picker=schemes.PickerArgs(gcmodel="affine"), chain_large=True)
    with pytest.raises(many.error, match="empty"):
        many.align_many([["ACGT" * 600, ""]], picker=schemes.PickerArgs(), chain_large=True)


def test_the_golden_file_regenerates(jobs, golden):
    import pin_oracle as P
    refmod = P.load_refmod(False)
    if refmod is None:
        pytest.skip("oracle/_ref/reveallib.so not built (make -C oracle refmod needs the reference's sources)")
    for name, kw in cl.SETS:
        for j, (cls, pair) in enumerate(jobs):
            an, T, first = cl.rem_align_recorded(list(pair), indexmod=refmod, **kw)
            assert (an, cl.sha(T)) == golden[name][j], (name, j, cls)
            if name == "default":
                assert first == golden["roots"][j], (j, cls)
    an, T, _ = cl.rem_align_recorded(list(cl.big_job()), indexmod=refmod, **cl.BIG_SET[1])
    assert (an, cl.sha(T)) == golden["big"][0]
