"""align_many with the reference's default picker, without a device: the job list of the GPU tests and its golden file (tests/golden/many_chain.json:
`rem.align` on the reference's own index, tools/gen_many_chain_golden.py), the admission rule of the shared launch, and the argument errors that come
before the library is asked for a device."""
import os
import sys

import pytest

import many_cases as mc
import many_chain_cases as cc
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many, schemes

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))


def as_bytes(pair):
    return [s.upper().encode() for s in pair]


@pytest.fixture(scope="module")
def jobs():
    return cc.jobs()


@pytest.fixture(scope="module")
def golden():
    return cc.load_golden()


def test_cases_are_deterministic_and_admitted(jobs):
    assert jobs == cc.jobs()
    assert len(jobs) == cc.N_CLASS + cc.N_REARRANGED + 2
    assert [c for c, _ in jobs[:cc.N_CLASS]] == [c for c, _ in mc.class_jobs(4)]
    assert sum(c == "rearranged" for c, _ in jobs) == cc.N_REARRANGED
    assert [len(a) + len(b) + 2 for c, (a, b) in jobs if c.startswith("full-")] == [2048, 2048]
    assert [n for n, _ in cc.SETS] == ["default", "wpen4", "wscore3", "star-avg", "star-med", "minl10", "minl1"]
    for name, kw in cc.SETS:
        args = cc.picker_args(kw)
        for cls, pair in jobs:
            assert many.takes_shared_launch(as_bytes(pair), picker=args, chain=True, minlength=kw["minlength"]), (name, cls)
            assert not many.takes_shared_launch(as_bytes(pair), picker=args, chain=False, minlength=kw["minlength"]), (name, cls)
            # (with a picker the other switches mean nothing)
            assert not many.takes_shared_launch(as_bytes(pair), multi=True, large=True, large_multi=True, wide=True, picker=args, minlength=kw["minlength"])


def test_golden_file_is_self_consistent(jobs, golden):
    """anchors of a job are disjoint and collinear on both sequences, lie inside them, and the upper-cased text lower-cased over them is the
    recorded final text"""
    for name, kw in cc.SETS:
        assert len(golden[name]) == len(jobs)
        for (cls, (a, b)), (anchors, sha) in zip(jobs, golden[name]):
            text = bytearray((a.upper() + "$" + b.upper() + "$").encode())
            la = len(a)
            assert anchors == sorted(anchors)
            by_a = sorted(anchors, key=lambda x: x[1][0])
            for k, (l, (pa, pb)) in enumerate(by_a):
                assert l >= 1 and 0 <= pa and pa + l <= la and la + 1 <= pb and pb + l <= len(text) - 1, (name, cls)
                assert text[pa:pa + l] == text[pb:pb + l], (name, cls)
                if k:
                    l0, (qa, qb) = by_a[k - 1]
                    assert qa + l0 <= pa and qb + l0 <= pb, (name, cls, "not disjoint and collinear")
            for l, (pa, pb) in anchors:
                text[pa:pa + l] = text[pa:pa + l].lower()
                text[pb:pb + l] = text[pb:pb + l].lower()
            assert cc.sha(bytes(text)) == sha, (name, cls)


def test_golden_file_differs_from_the_built_in_picker(jobs, golden):
    """what makes the fixture a test of the picker: on most `rearranged` jobs the longest-match picker chooses other anchors"""
    differ = 0
    for j, (cls, pair) in enumerate(jobs):
        if cls == "rearranged":
            want, _ = mc.oracle_job(as_bytes(pair), 20)
            differ += want != golden["default"][j][0]
    assert 2 * differ >= cc.N_REARRANGED, differ


def test_what_the_shared_launch_does_not_take():
    rng = __import__("random").Random(5)
    a = mc.rnd(rng, 1023)
    pair = [a.encode(), mc.mutate(rng, a, 0.01).encode()]
    args = schemes.PickerArgs(maxmums=10000)
    assert many.takes_shared_launch(pair, picker=args, chain=True)                                            # 2048 ranks
    assert not many.takes_shared_launch([pair[0] + b"A", pair[1]], picker=args, chain=True)                   # 2049 ranks
    small = [pair[0][:200], pair[1][:180]]
    assert many.takes_shared_launch(small, picker=args, chain=True)
    assert not many.takes_shared_launch(small, picker=schemes.PickerArgs(maxmums=10000, seedsize=30), chain=True)      # a seed could arise
    assert many.takes_shared_launch(small, picker=schemes.PickerArgs(maxmums=10000, seedsize=201), chain=True)
    assert many.takes_shared_launch(small, picker=schemes.PickerArgs(maxmums=10000, seedsize=0), chain=True)
    assert not many.takes_shared_launch(small, picker=schemes.PickerArgs(maxmums=10000, trim=False), chain=True)
    assert not many.takes_shared_launch(small, picker=schemes.PickerArgs(maxmums=5), chain=True)                       # the cap could bite
    assert many.takes_shared_launch(small, picker=schemes.PickerArgs(maxmums=180), chain=True)
    assert not many.takes_shared_launch(small, picker=schemes.PickerArgs(maxmums=179), chain=True)
    assert not many.takes_shared_launch(small, picker=args, chain=True, minlength=0)                                   # the p-value cut stays on the host
    assert not many.takes_shared_launch(small, picker=schemes.PickerArgs(maxmums=10000, wpen=-1), chain=True)
    assert not many.takes_shared_launch(small, picker=schemes.PickerArgs(maxmums=10000, wscore=many.CHAIN_WMAX + 1), chain=True)
    assert not many.takes_shared_launch(small + [small[0]], picker=args, chain=True)                                   # three sequences
    assert not many.takes_shared_launch([small[0], b"AC\0GT"], picker=args, chain=True)
    # without a picker nothing changes
    assert many.takes_shared_launch(small) and many.takes_shared_launch(small, chain=True)


@pytest.mark.parametrize("bad", [dict(maxdepth=3), dict(maxsize=100)])
def test_unsupported_picker_options_raise_before_any_device(bad, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(many, "Batch", no_device)
    with pytest.raises(many.error, match="maxbubblesize / maxdepth"):
        many.align_many([["ACGT" * 10, "ACGT" * 10]], picker=schemes.PickerArgs(**bad))
    with pytest.raises(many.error, match="gap cost model"):
        many.align_many([["ACGT" * 10, "ACGT" * 10]], picker=schemes.PickerArgs(gcmodel="affine"))


def test_a_sample_of_the_golden_regenerates(jobs, golden):
    import pin_oracle as P
    refmod = P.load_refmod(False)
    if refmod is None:
        pytest.skip("oracle/_ref/reveallib.so not built (make -C oracle refmod needs the reference's sources)")
    for name, kw in cc.SETS:
        for j in list(range(0, len(jobs), 9)) + [len(jobs) - 2, len(jobs) - 1]:
            an, T = cc.rem_align_job(list(jobs[j][1]), indexmod=refmod, **kw)
            assert (an, cc.sha(T)) == golden[name][j], (name, j, jobs[j][0])
